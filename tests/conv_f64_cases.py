"""Cases, float64 references, bounds and CPU emulations shared by tests/test_conv_f64_cpu.py (the proof, no GPU) and
tests/test_gpu_conv_f64.py (the kernels).  A plain module, not a test file.

tests/test_gpu_conv_exact.py feeds the conv kernels {-1, 0, +1}: exact in any order and under any rounding, hence blind
to everything that is about rounding -- a bf16-sized intermediate, a truncating store, a damaged low mantissa bit, a
statistic taken from the rounded tile.  tests/test_gpu_kernels.py uses general values under 1e-2 * max |ref|, which all
of those pass.  Here the operands carry full bf16 mantissas and every output element is held to the bracket
tests/parity.py derives (bf16_bracket) from the float64 convolution of the same operands.

Two draws per shape, both rounded to bf16:
  mixed   x, dy ~ U(-1, 1), w ~ U(-1, 1) / sqrt(Cin K K): signs, cancellation, low mantissa bits;
  pos     the absolute values of the same draw: no cancellation, so the magnitude sum A equals |ref| and the accumulation
          bound is terms * U32 RELATIVE (3.4e-5 at 576 terms, 2.7e-4 at 4608) against a bf16 spacing of 4-8e-3: nearly
          every bracket holds one value, at every K.  With mixed signs A / |ref| grows like sqrt(terms) and beyond, the
          bracket is several values wide at 4608 terms -- which is why both draws are needed.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.parity import U32, bf16_bracket, bf16_bracket_epilogue, conv_acc_bound

DRAWS = ("mixed", "pos")
# Floors of the decisive share (elements whose bracket holds ONE bf16 value), asserted on the float64 reference alone.
# pos: a bracket is wider than one value only where ref lies within b = terms * U32 * |ref| of a rounding boundary;
# boundaries are one spacing >= 2^-8 |ref| apart, so the expected share of such elements is at most
# 2 b / spacing <= 2 * 4608 * 2^-24 / 2^-8 = 0.14 at the longest K range used here: 0.85 holds with room at every case.
POS_DECISIVE_FLOOR = 0.85


def pos_decisive_floor(terms):
  """0.85 up to the 4608 terms it was derived for; beyond (the 5 x 5 layers of ClusterNet6c: 6400 terms in the forward
  of 256 -> 512 and the backward-data of 128 -> 256, 12800 in the backward-data of 256 -> 512) the same expression,
  1 - 2 terms 2^-24 / 2^-8, less the same margin of 0.01: 0.795 and 0.599."""
  return POS_DECISIVE_FLOOR if terms <= 4608 else 1.0 - 2.0 * terms * 2.0 ** -24 / 2.0 ** -8 - 0.01


# mixed, cases of <= 576 terms only: the float64 references of CONV_CASES give 0.960 / 0.975 at 64 / 128 terms and
# 0.544-0.559 at 576 (forward and backward-data alike); the floors are the smallest of those figures less a margin of
# 0.1 for another shape's draw.  Beyond 576 terms the share falls to 0.23 (1152) and 0 (4608): no floor, `pos` decides.
def mixed_decisive_floor(terms):
  return 0.86 if terms <= 128 else 0.44 if terms <= 576 else None


class Case(object):
  """nn.Conv2d(cin, cout, K, stride s, padding p, dilation d) on N images of H x W, PT border P."""

  def __init__(self, cin, cout, K, s, p, N, H, W=None, d=1, P=1, seed=0):
    self.cin, self.cout, self.K, self.s, self.p, self.N, self.H, self.W = cin, cout, K, s, p, N, H, (W or H)
    self.d, self.P, self.seed = d, P, seed

  def _key(self):
    return (self.cin, self.cout, self.K, self.s, self.p, self.N, self.H, self.W, self.d, self.P, self.seed)

  def __hash__(self):
    return hash(self._key())

  def __eq__(self, other):
    return isinstance(other, Case) and self._key() == other._key()

  def __repr__(self):
    return "%dto%d_k%ds%dp%dd%d_n%d_%dx%d_P%d" % (self.cin, self.cout, self.K, self.s, self.p, self.d, self.N, self.H,
                                                    self.W, self.P)

  @property
  def spec(self):
    from iic_amd import geom
    return geom.ConvSpec(self.cin, self.cout, self.K, self.s, self.p, self.d)

  @property
  def out_hw(self):
    o = lambda h: (h + 2 * self.p - self.d * (self.K - 1) - 1) // self.s + 1
    return o(self.H), o(self.W)

  # products per output element
  @property
  def terms_fwd(self):
    return self.K * self.K * self.cin

  @property
  def terms_bd(self):
    return self.K * self.K * self.cout

  @property
  def terms_wg(self):
    return self.N * self.out_hw[0] * self.out_hw[1]

  @property
  def count(self):
    """Output pixels per channel (the statistics' population)."""
    return self.terms_wg

  def kw(self):
    return dict(stride=self.s, padding=self.p, dilation=self.d)


def of(case_tuple, **kw):
  cin, cout, K, s, p, N, H = case_tuple
  return Case(cin, cout, K, s, p, N, H, **kw)


# Layer geometries of tests/conv_layer_cases.py that tests/test_gpu_kernels.py's CONV_CASES lack, for the brackets (the
# lattice of tests/test_gpu_conv_layers_exact.py is blind to rounding): the three 25-tap 5 x 5 layers of ClusterNet6c
# (PT border 2) at batches that leave a tail after whole tiles (M = 432, 180, 261), 512 -> 512 on a 3 x 3 plane where
# every pixel is a border pixel (M = 261), 64 -> 64 on 33 x 33 (the persistent kernel, M = 1089) and the stride-2
# 128 -> 256 on 17 x 17 (four parity classes of 81 / 72 / 72 / 64 rows per image).
LAYER_CASES = [Case(64, 128, 5, 1, 2, 3, 12, P=2), Case(128, 256, 5, 1, 2, 5, 6, P=2), Case(256, 512, 5, 1, 2, 29, 3, P=2),
               Case(512, 512, 3, 1, 1, 29, 3), Case(64, 64, 3, 1, 1, 1, 33), Case(128, 256, 3, 2, 1, 3, 17)]


def bf16(t):
  return t.to(torch.bfloat16).float()


def _unit(rng, shape, scale=1.0):
  return bf16(torch.from_numpy((rng.uniform(-1.0, 1.0, shape) * scale).astype(np.float32)))


@functools.lru_cache(maxsize=6)
def inputs(case, draw):
  """x, w, dy and the epilogue inputs prev, rg (like x, following the draw) and act (like x, always of mixed sign: the
  ReLU mask it gives keeps about half), float32 tensors holding bf16 values.  Shared, never modified."""
  assert draw in DRAWS
  rng = np.random.default_rng([case.seed, case.cin, case.cout, case.K, case.N, case.H, case.W])
  Ho, Wo = case.out_hw
  t = collections.OrderedDict()
  t["x"] = _unit(rng, (case.N, case.cin, case.H, case.W))
  t["w"] = _unit(rng, (case.cout, case.cin, case.K, case.K), 1.0 / np.sqrt(case.cin * case.K * case.K))
  t["dy"] = _unit(rng, (case.N, case.cout, Ho, Wo))
  t["prev"] = _unit(rng, (case.N, case.cin, case.H, case.W))
  t["rg"] = _unit(rng, (case.N, case.cin, case.H, case.W))
  act = _unit(rng, (case.N, case.cin, case.H, case.W))
  if draw == "pos":
    t = collections.OrderedDict((k, v.abs()) for k, v in t.items())
  t["act"] = act
  return t


# ---- float64 references: the value and the magnitude sum A (the same operation on |operand|, |operand|) --------------
def conv64(case, x, w):
  return F.conv2d(x.double(), w.double(), **case.kw())


def bd64(case, dy, w):
  return torch.nn.grad.conv2d_input((case.N, case.cin, case.H, case.W), w.double(), dy.double(), **case.kw())


def wg64(case, x, dy):
  return torch.nn.grad.conv2d_weight(x.double(), (case.cout, case.cin, case.K, case.K), dy.double(), **case.kw())


@functools.lru_cache(maxsize=6)
def ref_forward(case, draw):
  t = inputs(case, draw)
  return conv64(case, t["x"], t["w"]), conv64(case, t["x"].abs(), t["w"].abs())


@functools.lru_cache(maxsize=6)
def ref_backward_data(case, draw):
  t = inputs(case, draw)
  return bd64(case, t["dy"], t["w"]), bd64(case, t["dy"].abs(), t["w"].abs())


@functools.lru_cache(maxsize=6)
def ref_backward_weight(case, draw):
  t = inputs(case, draw)
  return wg64(case, t["x"], t["dy"]), wg64(case, t["x"].abs(), t["dy"].abs())


def forward_bracket(case, draw):
  """ref, b, lo, hi of the forward output."""
  ref, A = ref_forward(case, draw)
  b = conv_acc_bound(case.terms_fwd, A)
  return (ref, b) + bf16_bracket(ref, b)


def backward_data_bracket(case, draw):
  ref, A = ref_backward_data(case, draw)
  b = conv_acc_bound(case.terms_bd, A)
  return (ref, b) + bf16_bracket(ref, b)


def weight_gradient_bound(case, draw, nsplit, prev=None):
  """ref, tol of the fp32 weight gradient: N Ho Wo products, the fold of nsplit partials and (accumulate) the addition
  onto the previous dW, whose magnitude joins A: conv_acc_bound(N Ho Wo, A [+ |prev|], extra = nsplit + 1)."""
  ref, A = ref_backward_weight(case, draw)
  if prev is not None:
    ref, A = ref + prev.double(), A + prev.double().abs()
  return ref, conv_acc_bound(case.terms_wg, A, extra=nsplit + 1)


# The backward-data epilogues of igemm_store_tile (include/iic_hip.h IIC_ACC_*): name, keyword arguments of
# ops.conv_igemm less the tensors, which of (prev, rg, act) they read.
EPILOGUES = [
  ("accumulate", dict(accumulate=True), ("prev",)),
  ("res_grad+res_act", dict(), ("rg", "act")),
  ("premask+res_act", dict(premask=True), ("act",)),
  ("premask+res_grad", dict(premask=True), ("rg",)),
  ("premask+res_grad+res_act", dict(premask=True), ("rg", "act")),
  ("premask+accumulate+res_grad+res_act", dict(premask=True, accumulate=True), ("prev", "rg", "act")),
]


def epilogue_bracket(lo, hi, t, reads, premask):
  return bf16_bracket_epilogue(lo, hi, prev=t["prev"] if "prev" in reads else None,
                               res_grad=t["rg"] if "rg" in reads else None,
                               res_act=t["act"] if "act" in reads else None, premask=premask)


def decisive_share(lo, hi):
  return float((lo == hi).double().mean())


def stat_bounds(ref, b, count):
  """Tolerances of the per-channel BatchNorm cells S1 = sum y, S2 = sum y^2 (NCHW ref, reduced over N, H, W), which the
  kernels take from their fp32 accumulators a_i, |a_i - ref_i| <= b_i:
    |S1 - sum ref|   <= sum b_i                    (the accumulators' own error)
                        + count U32 sum |ref_i|    (fp32 partial sums per lane / wave / workgroup: every value passes
                                                    through fewer than `count` = N Ho Wo additions, each within U32 of a
                                                    partial sum that sum |a_i| bounds; the cells themselves are exact);
    |S2 - sum ref^2| <= sum (2 |ref_i| b_i + b_i^2)       (a_i^2 - ref_i^2 = (a_i - ref_i)(a_i + ref_i))
                        + U32 sum ref_i^2                  (one rounding of each product a_i * a_i; none if fused)
                        + count U32 sum ref_i^2            (the partial sums, as above).
  A partial never spans more than one tile of 256 rows and a few cross-lane steps, far fewer additions than `count`:
  that slack covers the second-order b_i inside sum |a_i|.  Statistics taken from the ROUNDED tile instead carry
  2^-9 |ref_i| of independent error per element and miss these bounds (tests/test_conv_f64_cpu.py, defect 4)."""
  dims = (0, 2, 3)
  a = ref.abs()
  tol1 = b.sum(dims) + count * U32 * a.sum(dims)
  tol2 = (2 * a * b + b * b).sum(dims) + (count + 1) * U32 * (ref * ref).sum(dims)
  return tol1, tol2


# ----------------------------------------------------------------------------------------------------------------------
# CPU emulations of what a kernel may legitimately do (fp32 accumulation in some order, one RNE store) and of seeded
# defects.  `parts` functions return the fp32 partial sums of a K range cut into chunks; fold() adds them in an order.
# ----------------------------------------------------------------------------------------------------------------------
def forward_parts(case, x, w, chunks):
  """fp32 partial forward outputs over `chunks` slices of the input channels (chunks = 1: plain fp32 F.conv2d)."""
  return [F.conv2d(x[:, g].contiguous(), w[:, g].contiguous(), **case.kw()) for g in torch.arange(case.cin).chunk(chunks)]


def backward_data_parts(case, dy, w, chunks):
  shape = (case.N, case.cin, case.H, case.W)
  return [torch.nn.grad.conv2d_input(shape, w[g].contiguous(), dy[:, g].contiguous(), **case.kw())
          for g in torch.arange(case.cout).chunk(chunks)]


def backward_weight_parts(case, x, dy, chunks):
  """Split-K of the weight gradient: the batch cut into `chunks` runs of images."""
  shape = (case.cout, case.cin, case.K, case.K)
  return [torch.nn.grad.conv2d_weight(x[g].contiguous(), shape, dy[g].contiguous(), **case.kw())
          for g in torch.arange(case.N).chunk(chunks)]


def fold(parts, order=None, on_acc=None):
  """fp32 sum of the partials in `order` (default: as listed); on_acc(acc) may damage the running sum (defect 5)."""
  order = list(range(len(parts))) if order is None else list(order)
  acc = parts[order[0]].clone()
  if on_acc:
    acc = on_acc(acc)
  for i in order[1:]:
    acc = acc + parts[i]
    if on_acc:
      acc = on_acc(acc)
  return acc


def store_rne(acc):
  return acc.to(torch.bfloat16).float()        # torch's float32 -> bfloat16 rounds to nearest-even


def store_truncating(acc):
  """Defect 1: the bf16 store drops the low 16 bits instead of rounding."""
  return (acc.contiguous().view(torch.int32) & -65536).view(torch.float32)


def clear_low_mantissa_bit(t):
  """Defect 3: the lowest of the 7 stored bf16 mantissa bits of an operand cleared."""
  return (t.contiguous().view(torch.int32) & ~(1 << 16)).view(torch.float32)


def shorten_mantissa(acc, bits=10):
  """Defect 5: an fp32 value cut to `bits` stored mantissa bits (truncation)."""
  return (acc.contiguous().view(torch.int32) & ~((1 << (23 - bits)) - 1)).view(torch.float32)


def epilogue_emulated(tile, t, reads, premask):
  """igemm_store_tile on a bf16-valued fp32 tile, in the kernel's order and precision (csrc/conv_tile.h:164-199)."""
  f = tile.clone()
  if "prev" in reads:
    f = f + t["prev"]
  keep = (t["act"] > 0) if "act" in reads else None
  if "rg" in reads:
    f = f + (t["rg"] if (premask or keep is None) else torch.where(keep, t["rg"], torch.zeros_like(f)))
  if premask and keep is not None:
    f = torch.where(keep, f, torch.zeros_like(f))
  return store_rne(f)


def stats_of(values):
  """[2, C] float64: per-channel sums of the fp32 values and of their fp32 squares, the sums themselves exact (the
  fixed-point cells)."""
  sq = values * values
  return torch.stack([values.double().sum((0, 2, 3)), sq.double().sum((0, 2, 3))])


def stats_of_fp32_sums(values):
  """The same with the sums carried in fp32 (torch's own reduction order)."""
  return torch.stack([values.sum((0, 2, 3)), (values * values).sum((0, 2, 3))]).double()


# ---- the criteria the suite already had ----------------------------------------------------------------------------
def old_accepts(got, ref, rel=1e-2):
  """tests/test_gpu_kernels.py: max |got - ref| <= rel * max |ref| (1e-2 forward / backward-data, 3e-3 weight
  gradient), against an fp32 reference there; the float64 one here differs from it by ~1e-6 of the scale."""
  return float((got.double() - ref.double()).abs().max()) <= rel * float(ref.abs().max())


def old_accepts_stats(st, ref, count):
  """tests/test_gpu_kernels.py _conv_forward_and_stats: the means within atol = 2e-3 * scale; the mean squares within
  rtol 2e-3 + atol 1e-4 * scale^2."""
  scale = float(ref.abs().max())
  m1, m2 = ref.mean((0, 2, 3)), (ref * ref).mean((0, 2, 3))
  ok1 = bool(((st[0] / count - m1).abs() <= 2e-3 * scale).all())
  ok2 = bool(((st[1] / count - m2).abs() <= 1e-4 * scale * scale + 2e-3 * m2.abs()).all())
  return ok1 and ok2
