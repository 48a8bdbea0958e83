"""Cases, draws, float64 references, derived bounds and the numpy emulation shared by tests/test_triplets_cpu.py (the
proof, no GPU) and tests/test_gpu_triplets.py (csrc/triplets.hip).  A plain module, not a test file.

The loss (code/utils/cluster/baselines/triplets.py:231-238; "elementwise_mean" divides by N k).  Logits a (orig), b (pos),
c (neg), all [N, k]:
  lo = a - lse(a)   lp = b - lse(b)   lq = c - lse(c)   p = exp(lp)   q = exp(lq)
  tp_n = sum_j p (lp - lo)      tq_n = sum_j q (lq - lo)
  loss = sum_n (tp_n - tq_n) / (N k)
  d_a  = (q - p) / (N k)
  d_b  =  p ((lp - lo) - tp_n) / (N k)
  d_c  = -q ((lq - lo) - tq_n) / (N k)
`closed64` is this closed form in torch float64, written from the formulas above and sharing nothing with iic_amd/;
`autograd64` is F.kl_div(log_softmax(a), softmax(b), "mean") - F.kl_div(log_softmax(a), softmax(c), "mean") under float64
autograd.  The two agree on every case of CASES (asserted in test_triplets_cpu.py); at the spread-1600 case torch's
target gradients are 0 * (-inf) = NaN and only the closed form is a reference.

Bounds.  The kernel evaluates the closed form in float64 and rounds every output to fp32 once, so per output
  tol = U32 |ref| + 2 e64 + SUBNORMAL
with e64 the float64 evaluation error of the closed form (below), charged twice: once for the kernel, once for the
reference, which evaluates the same expressions in another order.  u = U64 = 2^-53 per float64 operation; exp and log are
charged EXP_ULPS units each (the device library and numpy / torch document 1 ulp = at most 2 u; 4 leaves the same again
in hand, as tests/sup_head_cases.py charges fp32 expf).  With E = EXP_ULPS:
  lse(x) = m + log s, s = sum_j exp(x_j - m), m = max x (exact)
     x_j - m: u |x_j - m|;  e_j = exp(.): u (|x_j - m| e_j + E e_j) <= u (0.37 + E e_j);  k - 1 additions of positive terms:
     (k - 1) u s;  s >= 1, so  |err s| / s <= u (1.37 k + E);  log: + E u log k;  the addition: + u |lse|
     L(x) = u (1.37 k + E + E log k + |lse|)
  lo = a - lse(a)        e_lo = L(a) + u |lo|              (likewise e_lp, e_lq)
  p  = exp(lp)           relative r_p = e_lp + E u
  d  = lp - lo           e_d = e_lp + e_lo + u |d|
  term = p d             e_term = |term| (r_p + u) + p e_d
  tp = sum_j term        e_tp = sum_j e_term + (k - 1) u sum_j |term|        (any order of the k - 1 additions)
  r_n = tp - tq          e_r = e_tp + e_tq + u |r_n|
  loss                   [sum_n e_r + (N - 1) u sum_n |r_n|] / (N k) + u |loss|
  d_a                    [p r_p + q r_q + u |q - p|] / (N k) + u |d_a|
  d_b                    g = d - tp: e_g = e_d + e_tp + u |g|;  [|p g| (r_p + u) + p e_g] / (N k) + u |d_b|      (d_c alike)
SUBNORMAL is one fp32 subnormal spacing, 2^-149: iic_amd/csrc/Makefile passes neither -ffast-math nor
-fgpu-flush-denormals-to-zero, and without them hipcc keeps fp32 denormals on gfx950 (`flushes_denormals` reads the
flags; with a flushing build the term would be 2^-126).
"""
import collections
import functools
import os
import re
import warnings

import numpy as np
import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
EXP_ULPS = 4.0
SLACK = 1.0 + 2.0 ** -10          # second-order terms (products of two u-sized errors)
ROWS_PER_WG = 4                   # TR_ROWS of csrc/triplets.hip: rows (waves) per workgroup, one float64 partial each
WIDE_SPREAD = 160.0               # exp(-160) is 0 in fp32 (below 2^-149) and 3e-70 in float64
HUGE_SPREAD = 1600.0              # exp(-1600) is 0 in float64 too: torch's target gradients are NaN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "name N k")
CASES = [Case("1x1", 1, 1), Case("1x2", 1, 2), Case("3x10", 3, 10), Case("5x63", 5, 63), Case("5x64", 5, 64),
         Case("5x65", 5, 65), Case("3x129", 3, 129), Case("2x1024", 2, 1024), Case("700x10", 700, 10),
         Case("wg_plus_one", 16 * ROWS_PER_WG + 1, 7),      # one row more than 16 whole workgroups
         Case("4099x3", 4099, 3),                           # thousands of rows: the finisher's runs hold several partials
         Case("strided", 300, 10)]                          # read as a [300, 10] view of [300, 15] on the device
STRIDED_LD = 15
HUGE_CASE = Case("spread1600", 3, 10)


def case_id(c):
  return c.name


def flushes_denormals():
  """Whether the build's flags flush fp32 denormals (they do not: see the module docstring)."""
  text = open(os.path.join(ROOT, "iic_amd", "csrc", "Makefile")).read()
  return re.search(r"-ffast-math|-fgpu-flush-denormals-to-zero|-fcuda-flush-denormals-to-zero|-cl-denorms-are-zero",
                   text) is not None


def subnormal_term():
  return 2.0 ** -126 if flushes_denormals() else 2.0 ** -149


def wide_row(case):
  """Index of the row that carries the wide linspace, or None (a single-row case keeps its normal draw)."""
  return case.N // 2 if case.N >= 2 and case.k >= 2 else None


@functools.lru_cache(maxsize=None)
def inputs(case):
  """(a, b, c): float32 [N, k] host tensors drawn N(0, 3^2); row N // 2 of b is linspace(-s/2, s/2), of c the reverse
  (s = 160, or 1600 for HUGE_CASE).  Shared, never modified."""
  rng = np.random.default_rng([31, case.N, case.k, len(case.name)])
  a, b, c = (torch.from_numpy((rng.standard_normal((case.N, case.k)) * 3).astype(np.float32)) for _ in range(3))
  r = wide_row(case)
  if r is not None:
    s = HUGE_SPREAD if case.name == HUGE_CASE.name else WIDE_SPREAD
    b[r] = torch.linspace(-s / 2, s / 2, case.k)
    c[r] = torch.linspace(s / 2, -s / 2, case.k)
  return a, b, c


# ---- float64 references ------------------------------------------------------------------------------------------------
def closed64(a, b, c):
  """The closed form in float64: dict of loss (0-d), d_a, d_b, d_c and the intermediates the bounds use."""
  a, b, c = a.double(), b.double(), c.double()
  N, k = a.shape
  lse = lambda x: torch.logsumexp(x, dim=1, keepdim=True)
  lo, lp, lq = a - lse(a), b - lse(b), c - lse(c)
  p, q = torch.exp(lp), torch.exp(lq)
  dp, dq = lp - lo, lq - lo
  tp, tq = (p * dp).sum(1, keepdim=True), (q * dq).sum(1, keepdim=True)
  nk = float(N * k)
  return dict(loss=(tp - tq).sum() / nk, d_a=(q - p) / nk, d_b=p * (dp - tp) / nk, d_c=-q * (dq - tq) / nk,
              lo=lo, lp=lp, lq=lq, p=p, q=q, dp=dp, dq=dq, tp=tp, tq=tq)


def autograd64(a, b, c):
  """The reference's composition under float64 autograd: (loss, d_a, d_b, d_c)."""
  F = torch.nn.functional
  a, b, c = (t.double().clone().requires_grad_(True) for t in (a, b, c))
  orig = F.log_softmax(a, dim=1)
  with warnings.catch_warnings():
    # reduction="mean" is what the reference's "elementwise_mean" became (the sum over N k); torch warns that it is
    # not the KL divergence's own "batchmean"
    warnings.simplefilter("ignore")
    loss = F.kl_div(orig, F.softmax(b, dim=1), reduction="mean") - F.kl_div(orig, F.softmax(c, dim=1), reduction="mean")
  loss.backward()
  return loss.detach(), a.grad, b.grad, c.grad


@functools.lru_cache(maxsize=None)
def refs(case):
  return closed64(*inputs(case))


# ---- bounds ------------------------------------------------------------------------------------------------------------
def _L(x):
  x = x.double()
  k = x.shape[1]
  lse = torch.logsumexp(x, dim=1, keepdim=True)
  return U64 * (1.37 * k + EXP_ULPS + EXP_ULPS * np.log(k) + lse.abs())


def eval_error64(a, b, c, r=None):
  """e64 per output (dict loss, d_a, d_b, d_c): the float64 evaluation error derived in the module docstring."""
  r = closed64(a, b, c) if r is None else r
  N, k = a.shape
  nk, u = float(N * k), U64
  e_lo, e_lp, e_lq = _L(a) + u * r["lo"].abs(), _L(b) + u * r["lp"].abs(), _L(c) + u * r["lq"].abs()
  out = {}
  e_t, e_dd, rr = {}, {}, {}
  for name, w, l, d, e_l in (("p", r["p"], r["lp"], r["dp"], e_lp), ("q", r["q"], r["lq"], r["dq"], e_lq)):
    rel = e_l + EXP_ULPS * u
    e_d = e_l + e_lo + u * d.abs()
    term = (w * d).abs()
    e_term = term * (rel + u) + w * e_d
    e_t[name] = e_term.sum(1, keepdim=True) + (k - 1) * u * term.sum(1, keepdim=True)
    e_dd[name], rr[name] = e_d, rel
  row = r["tp"] - r["tq"]
  e_r = e_t["p"] + e_t["q"] + u * row.abs()
  out["loss"] = (e_r.sum() + (N - 1) * u * row.abs().sum()) / nk + u * r["loss"].abs()
  out["d_a"] = (r["p"] * rr["p"] + r["q"] * rr["q"] + u * (r["q"] - r["p"]).abs()) / nk + u * r["d_a"].abs()
  for name, w, d, t, key in (("p", r["p"], r["dp"], r["tp"], "d_b"), ("q", r["q"], r["dq"], r["tq"], "d_c")):
    g = d - t
    e_g = e_dd[name] + e_t[name] + u * g.abs()
    out[key] = ((w * g).abs() * (rr[name] + u) + w * e_g) / nk + u * r[key].abs()
  return out


def bounds(a, b, c, r=None):
  """tol per output: U32 |ref| + 2 e64 + one fp32 subnormal spacing, times SLACK."""
  r = closed64(a, b, c) if r is None else r
  e = eval_error64(a, b, c, r)
  sub = subnormal_term()
  return {key: (U32 * r[key].abs() + 2.0 * e[key] + sub) * SLACK for key in ("loss", "d_a", "d_b", "d_c")}


@functools.lru_cache(maxsize=None)
def case_bounds(case):
  return bounds(*inputs(case), r=refs(case))


def outside(got, ref, tol):
  """Number of elements that are not within tol of ref (a non-finite value is outside)."""
  err = (torch.as_tensor(got).double() - ref.double()).abs()
  return int((~(err <= tol)).sum())


def worst(got, ref, tol):
  err = (torch.as_tensor(got).double() - ref.double()).abs()
  return float((err / tol).nan_to_num(nan=float("inf")).max())


# ---- numpy emulation of the kernel's arithmetic ----------------------------------------------------------------------
def _wave_sum(v, k):
  """[N, k] float64 -> [N]: lane j adds classes j, j + 64, .. in that order, then the 64 lanes fold in the xor butterfly
  (offsets 32, 16, .., 1) -- the order of tr_lse / tr_kl_row."""
  N = v.shape[0]
  T = (k + 63) // 64
  pad = np.zeros((N, T * 64))
  pad[:, :k] = v
  lanes = np.zeros((N, 64))
  for t in range(T):
    lanes = lanes + pad[:, t * 64:(t + 1) * 64]
  idx = np.arange(64)
  for o in (32, 16, 8, 4, 2, 1):
    lanes = lanes + lanes[:, idx ^ o]
  return lanes[:, 0]


def emulate(a, b, c, defect=None, defect_rows=None):
  """The kernel's arithmetic in numpy float64 with its summation orders and one fp32 rounding per output: dict of
  float32 loss [()], d_a, d_b, d_c.  `defect` seeds one wrong step (in `defect_rows`, default every row):
    "fp32_exp"   p and q from an fp32 exp of the fp32-rounded log-probability
    "log_exp"    log p taken as log(softmax) in fp32, as the torch composition on fp32 tensors has it
    "log_exp64"  the same in float64
    "div_n"      division by N instead of N k
    "sign_dc"    d_c with the wrong sign"""
  a, b, c = (np.asarray(t, dtype=np.float32) for t in (a, b, c))
  N, k = a.shape
  rows = np.ones(N, bool) if defect_rows is None else np.isin(np.arange(N), defect_rows)

  def lse(x):
    m = x.max(1).astype(np.float64)
    with np.errstate(all="ignore"):
      return m + np.log(_wave_sum(np.exp(x.astype(np.float64) - m[:, None]), k))

  def logp(x):
    l = x.astype(np.float64) - lse(x)[:, None]
    if defect in ("log_exp", "log_exp64"):
      dt = np.float32 if defect == "log_exp" else np.float64
      xs = x.astype(dt)
      e = np.exp(xs - xs.max(1, keepdims=True))
      with np.errstate(all="ignore"):
        bad = np.log(e / e.sum(1, keepdims=True, dtype=dt)).astype(np.float64)
      l = np.where(rows[:, None], bad, l)
    return l
  lo = a.astype(np.float64) - lse(a)[:, None]
  res = {}
  terms = {}
  for name, x in (("p", b), ("q", c)):
    l = logp(x)
    with np.errstate(all="ignore"):
      w = np.exp(l)
      if defect == "fp32_exp":
        w = np.where(rows[:, None], np.exp(l.astype(np.float32)).astype(np.float64), w)
      d = l - lo
      term = np.where(np.isneginf(l), 0.0 * lo, w * d)
    terms[name] = (w, d, _wave_sum(term, k))
  (p, dp, tp), (q, dq, tq) = terms["p"], terms["q"]
  nk = float(N) if defect == "div_n" else float(N) * float(k)
  with np.errstate(all="ignore"):
    r = tp - tq
    part = np.zeros(((N + ROWS_PER_WG - 1) // ROWS_PER_WG, ROWS_PER_WG))
    part.reshape(-1)[:N] = r
    partials = np.zeros(part.shape[0])
    for i in range(ROWS_PER_WG):
      partials = partials + part[:, i]
    W = partials.shape[0]
    per = (W + 255) // 256
    total = 0.0
    for t in range(256):
      run = 0.0
      for v in partials[t * per:(t + 1) * per]:
        run += v
      total += run
    res["loss"] = np.float32(total / nk)
    res["d_a"] = ((q - p) / nk).astype(np.float32)
    res["d_b"] = (p * (dp - tp[:, None]) / nk).astype(np.float32)
    res["d_c"] = -(q * (dq - tq[:, None]) / nk).astype(np.float32)
    if defect == "sign_dc":
      res["d_c"] = -res["d_c"]
  return res


# ---- triplets_eval restated in numpy (baselines/triplets.py:176-228) ---------------------------------------------------
def eval_np(preds, targets, gt_k):
  """(acc, mass [1, gt_k], per_class_acc [1, gt_k]) as the reference computes them from flat predictions and targets:
  Hungarian match on num_samples - num_correct, predictions rewritten through the match, per-class flags."""
  from scipy.optimize import linear_sum_assignment
  preds, targets = np.asarray(preds).astype(np.int64), np.asarray(targets).astype(np.int64)
  n = preds.shape[0]
  num_correct = np.zeros((gt_k, gt_k))
  for c1 in range(gt_k):
    for c2 in range(gt_k):
      num_correct[c1, c2] = int(((preds == c1) * (targets == c2)).sum())
  match = list(zip(*linear_sum_assignment(n - num_correct)))
  found = np.zeros(gt_k)
  reordered = np.zeros(n, dtype=np.int64)
  for pred_i, target_i in match:
    reordered[preds == pred_i] = target_i
    found[pred_i] = 1
  assert found.sum() == gt_k
  mass, per_class_acc = np.zeros((1, gt_k)), np.zeros((1, gt_k))
  for cls in range(gt_k):
    flags, actual = reordered == cls, targets == cls
    mass[0, cls] = flags.sum()
    per_class_acc[0, cls] = (flags * actual).sum()
  return int((reordered == targets).sum()) / float(n), mass, per_class_acc


def eval_batches(gt_k=4, sizes=(8, 8, 5), seed=5, output_k=None):
  """Logit batches [rows, output_k] and int64 target batches for the evaluation tests: targets follow the arg-max class
  two times in three; row 3 of batch 0 holds an exact tie between classes 1 and 3 (the lower index wins)."""
  output_k = gt_k if output_k is None else output_k
  rng = np.random.default_rng([32, gt_k, output_k, seed])
  logits, targets = [], []
  for bi, n in enumerate(sizes):
    lg = (rng.standard_normal((n, output_k)) * 2).astype(np.float32)
    if bi == 0:
      lg[3] = np.minimum(lg[3], 1.0)
      lg[3, 1] = lg[3, 3] = 2.5
    am = lg.argmax(1)
    tg = np.where(rng.random(n) < 0.67, (am + 1) % gt_k, rng.integers(0, gt_k, n)).astype(np.int64)
    logits.append(lg)
    targets.append(tg)
  return logits, targets
