"""Helpers shared by the float64 parity tests (tests/test_gpu_kernels_f64.py, tests/test_gpu_bn_bf16.py and the CPU proof of
the latter's bounds, tests/test_bn_bf16_cpu.py; the convolution and first-layer files named further down): direct calls of the C entry points, bit / bound comparisons, PT tensors
with a sentinel border and the mask inputs.  A plain module, not a test file: nothing here needs a GPU at import.

Tolerances are derived, not tuned: U32 = 2^-24 per fp32 operation and U16 = 2^-8 per bf16 store -- one unit in the last
place each, so neither round-to-nearest nor truncation is presumed for an intermediate."""
import numpy as np
import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8
SENTINEL = 7.0

# worst |err| / bound seen per family, for callers of assert_within that name one (LAB.md records them)
WORST = {}


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


def call(name, *args):
  from iic_amd import _lib
  rc = getattr(_lib.lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], _lib.stream_ptr())
  torch.cuda.synchronize()
  return rc


def ok(name, *args):
  from iic_amd import _lib
  _lib.check(call(name, *args), name)


def bits(t):
  t = t.detach().cpu().contiguous()
  return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits(got, want, what):
  got, want = bits(got), bits(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  bad = got != want
  assert not bool(bad.any()), "%s: %d elements differ, first at %s" % (what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]))


def assert_within(got, ref, tol, what, family=None):
  got, ref, tol = got.detach().cpu().double(), ref.double(), torch.as_tensor(tol).double()
  err = (got - ref).abs()
  bad = ~(err <= tol)
  worst = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
  if family is not None:
    WORST[family] = max(WORST.get(family, 0.0), worst)
  assert not bool(bad.any()), "%s: %d elements outside the bound; worst |err| / bound = %g" % (what, int(bad.sum()), worst)


# ----------------------------------------------------------------------------------------------------------------------
# Convolutions: an accumulation bound and, for a bf16 store, the bracket it implies (tests/conv_f64_cases.py,
# tests/test_conv_f64_cpu.py, tests/test_gpu_conv_f64.py, tests/test_gpu_p64_forms.py)
# ----------------------------------------------------------------------------------------------------------------------
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


def conv_acc_bound(terms, A, extra=0):
  """|fp32 accumulator - exact sum| for a sum of `terms` products of bf16 operands, accumulated in fp32 in any order and
  grouping: the products are exact in fp32 (8 x 8 significant bits), each of the at most `terms` additions rounds a
  partial sum whose magnitude is at most A = sum |operand| |operand| (the same convolution applied to the magnitudes,
  in float64), so each costs at most U32 * A -- whichever way it rounds.  `extra` counts further fp32 additions of
  partial results of the same sum (the split-K fold of the weight gradient, the addition onto a previous dW, whose
  magnitude the caller adds to A).  terms: forward taps * Cin; backward-data taps * Cout (an upper bound: a stride-2
  parity class uses fewer); weight gradient N * Ho * Wo."""
  return (terms + extra) * U32 * A


def bf16_rne(v):
  """float64 -> the nearest bf16 value, ties to even, as float64, in ONE rounding (torch's double -> bfloat16 passes
  through float32 and so rounds twice).  Subnormal bf16 values (spacing 2^-133) and overflow to inf included; inf and
  NaN pass through."""
  v = torch.as_tensor(v, dtype=torch.float64)
  fin = torch.isfinite(v)
  z = torch.where(fin, v, torch.zeros_like(v))
  q = bf16_spacing(z)
  r = torch.round(z / q) * q                              # (z / q is exact; torch.round is half-to-even)
  r = torch.where(r.abs() > BF16_MAX, torch.sign(r) * float("inf"), r)
  return torch.where(fin, r, v)


def bf16_spacing(v):
  """Distance between neighbouring bf16 values at |v| (float64)."""
  v = torch.as_tensor(v, dtype=torch.float64)
  z = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
  _, e = torch.frexp(z)                                   # |z| in [2^(e-1), 2^e): 8 significant bits end at 2^(e-8)
  e = torch.where(z == 0, torch.full_like(e, -125), e)
  return torch.ldexp(torch.ones_like(v), e.clamp(min=-125) - 8)


def bf16_bracket(ref, b):
  """(lo, hi) = (bf16_rne(ref - b), bf16_rne(ref + b)), float64 tensors holding bf16 values.

  Round-to-nearest-even is monotone: a kernel whose fp32 accumulator lies within b of the float64 reference and whose
  store rounds it to nearest-even (v_cvt_pk_bf16_f32: csrc/common.h:205-213, f32_to_bf16 / pack_bf16x2) must store a
  value in [lo, hi]; lo <= got <= hi is the whole assertion, no tolerance is tuned.  Where b is far below one bf16
  spacing the bracket holds a single value (`decisive`): the check is bit-exact there and rejects a truncating store
  and any intermediate error of bf16 size.  ref is float64 and bf16_rne rounds once, so no double rounding enters.

  The rounding points of the conv kernels, as their code has them:
    * accumulators -> bf16 tile in LDS, RNE: csrc/conv_igemm.hip:257, csrc/conv_igemm_bd.hip:442,
      csrc/conv_igemm_p64.hip:453 (f32_to_bf16), csrc/conv_igemm_pw.hip:545 (pack_bf16x2);
    * the BatchNorm statistics are taken from the fp32 accumulators BEFORE that rounding: csrc/conv_igemm.hip:215-248,
      csrc/conv_igemm_bd.hip:410-432, csrc/conv_igemm_p64.hip:440 / 498, csrc/conv_igemm_pw.hip:517-521 / 589 (per-lane
      fp32 partial sums, then the exact fixed-point cells of csrc/common.h:141-155);
    * the epilogue igemm_store_tile (csrc/conv_tile.h:164-199; csrc/conv_igemm_pw.hip:113-178 repeats it) widens the
      rounded tile to fp32, adds the previous contents (:169-173), then the residual gradient (:175-179 with
      IIC_ACC_PREMASK, :188-195 without, where the ReLU mask gates the residual only), zeroes masked elements (:180-187)
      and rounds ONCE more (:197, pack_bf16x2).  With no epilogue input the tile's bits are stored as they are (:200).
  bf16_bracket_epilogue carries the bracket through those steps."""
  ref, b = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
  return bf16_rne(ref - b), bf16_rne(ref + b)


def bf16_bracket_epilogue(lo, hi, prev=None, res_grad=None, res_act=None, premask=False):
  """The bracket of the tile, carried through igemm_store_tile (bf16_bracket's docstring lists its steps).  Every step is
  non-decreasing in the tile value t: a rounded fp32 addition of a fixed number is, the mask is (it maps to 0 or keeps),
  and so is the final RNE.  So with t in [lo, hi] the stored value lies in [lo2, hi2],
    lo2 = bf16_rne(lo + prev + rg - 3 U32 mag),   hi2 = bf16_rne(hi + prev + rg + 3 U32 mag),
  mag = |t| + |prev| + |rg| at the respective end: at most two fp32 additions, each within U32 of a partial sum that mag
  bounds, in either rounding direction -- 3 leaves one in hand.  rg = res_grad, gated by (res_act > 0) when premask is
  off; with premask on the whole element is exactly zero where res_act <= 0 (or is NaN).  All arguments NCHW, float64 or
  convertible, the epilogue inputs holding bf16 values."""
  z = torch.zeros_like(lo)
  prev = z if prev is None else prev.double()
  rg = z if res_grad is None else res_grad.double()
  keep = None if res_act is None else (res_act.double() > 0)
  if keep is not None and not premask:
    rg = torch.where(keep, rg, z)
  out = []
  for t, sign in ((lo, -1.0), (hi, 1.0)):
    mag = t.abs() + prev.abs() + rg.abs()
    v = bf16_rne(t + prev + rg + sign * 3 * U32 * mag)
    if keep is not None and premask:
      v = torch.where(keep, v, z)
    out.append(v)
  return out[0], out[1]


def assert_in_bracket(got, lo, hi, what, family=None, ref=None, b=None):
  """lo <= got <= hi element-wise (NaN fails).  With `family`, WORST[family] keeps two figures: `ratio`, the worst
  |got - ref| / (b + bf16 spacing at ref) (ref, b: the float64 reference and the accumulation bound the bracket was made
  from; a value inside its bracket stays below 1.5), and `decisive`, the smallest share of elements with lo == hi over
  the calls -- that one from the reference alone."""
  got, lo, hi = got.detach().cpu().double(), lo.double(), hi.double()
  assert got.shape == lo.shape == hi.shape, (what, got.shape, lo.shape, hi.shape)
  bad = ~((lo <= got) & (got <= hi))
  if family is not None:
    w = WORST.setdefault(family, {"ratio": 0.0, "decisive": 1.0, "elements": 0})
    w["decisive"] = min(w["decisive"], float((lo == hi).double().mean()))
    w["elements"] += got.numel()
    if ref is not None:
      den = torch.as_tensor(b, dtype=torch.float64) + bf16_spacing(ref)
      w["ratio"] = max(w["ratio"], float(((got - ref.double()).abs() / den).nan_to_num(nan=float("inf")).max()))
  if bool(bad.any()):
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError("%s: %d of %d elements outside their bf16 bracket; first at %s: got %r, bracket [%r, %r]" % (
      what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(lo[idx]), float(hi[idx])))


def outside_share(got, lo, hi):
  """Share of elements outside [lo, hi] (the CPU proof's rejection rates)."""
  got = got.detach().cpu().double()
  return float((~((lo <= got) & (got <= hi))).double().mean())


def rnd(rng, *shape):
  return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def pt_of(x_nhwc, P, dtype, fill=0.0):
  """[N, H, W, C] interior -> PT tensor [N, H+2P, W+2P, C] on the GPU, border = fill."""
  n, h, w, c = x_nhwc.shape
  out = torch.full((n, h + 2 * P, w + 2 * P, c), fill, dtype=dtype)
  out[:, P:P + h, P:P + w] = x_nhwc.to(dtype)
  return out.to(dev())


def interior(pt, P):
  return pt[:, P:pt.shape[1] - P, P:pt.shape[2] - P].cpu()


def assert_border(pt, P, value, what):
  m = torch.ones(pt.shape[1:3], dtype=torch.bool)
  m[P:pt.shape[1] - P, P:pt.shape[2] - P] = False
  b = pt.cpu().float()[:, m]
  assert bool((b == value).all()), "%s: the PT border was written" % what


def _mask_act(rng, N, H, W, C):
  act = rnd(rng, N, H, W, C)
  flat = act.view(-1)
  flat[0::7] = 0.0
  flat[1::7] = -0.0
  flat[2::7] = -abs(flat[2::7]) - 0.5
  return act


def _pow2_coef(rng, C):
  """scale, shift on powers of two / small dyadics: with y on multiples of 1/8 the mask expression scale*y + shift is
  exact in fp32, fused or not."""
  return torch.stack([torch.from_numpy(rng.choice([0.5, 1.0, 2.0, -1.0, -0.5], C)),
                      torch.from_numpy(rng.choice([0.0, 0.25, -0.25, 0.5, -1.0], C))]).float()


def _masked_g(dout, act, y, mcoef, mode):
  if mode == "act":
    return torch.where(act > 0, dout, torch.zeros_like(dout))
  if mode == "mask_coef":
    return torch.where(y * mcoef[0] + mcoef[1] > 0, dout, torch.zeros_like(dout))
  return dout


# ----------------------------------------------------------------------------------------------------------------------
# Exact-fp32 matrix pipe (stem, first conv, seg head): an accumulation bound for fp32 x fp32 products and the bracket of
# "affine, ReLU, 2x2/2 max-pool with padding 1, one RNE store" (tests/first_layer_f64_cases.py,
# tests/test_first_layer_f64_cpu.py, tests/test_gpu_first_layer_f64.py)
# ----------------------------------------------------------------------------------------------------------------------
def fma_acc_bound(terms, A, extra=0):
  """|fp32 accumulator - exact sum| for a sum of `terms` products of fp32 operands (a bf16 operand widened exactly is
  one), accumulated in fp32 in any order and grouping, A = sum |operand| |operand| (the same operation on the
  magnitudes, in float64):  n u / (1 - n u) * A,  u = U32 = 2^-24 (round to nearest), n = terms + extra + 1.

  Derivation.  Write the computed sum as a binary tree whose leaves are the products p_i and whose inner nodes are fp32
  additions (a chain is the degenerate tree; an accumulator that starts at zero adds 0 + p exactly; a fold of per-wave,
  per-workgroup or split-K partials only joins subtrees).  A tree over `terms` leaves has terms - 1 inner nodes, so a leaf
  lies under at most terms - 1 additions, each of which multiplies what is below it by (1 + d), |d| <= u:
    computed = sum p_i prod_{j over i} (1 + d_j),   |computed - sum p_i| <= ((1 + u)^(terms-1) - 1) sum |p_i|.
  * Fused (v_mfma_f32_*_f32 as an fmaf chain, which the kernels' headers state but no test establishes): a step rounds
    p + partial once -- that is the addition above, and the products carry no rounding of their own.
  * Not fused: every product is rounded first, p_i (1 + e_i), one more factor per leaf.  ALL the product roundings
    together cost at most u sum |p_i| = u A -- one more unit of n, not one per term -- which is the `+ 1`: the bound
    therefore holds for both, and nothing here presumes the fused form.
  * `extra`: further fp32 additions that a value passes through and that are not joins of partials of this sum (the
    acc + acc2 join of two chains is a join and needs none; the addition onto a previous result, a bias, or a fold the
    caller prefers to count apart do).
  (1 + u)^n - 1 <= n u / (1 - n u) for n u < 1 (Higham, Accuracy and Stability, lemma 3.1): second-order terms
  included, so the bound also holds at the 40 000 terms of a 200 x 200 weight gradient."""
  n = terms + extra + 1
  assert n * U32 < 1
  return (n * U32 / (1.0 - n * U32)) * A


def affine_bound(y, b, sc, sh):
  """z = sc y + sh in float64 and bz with |fp32 z - z| <= bz for the kernel's z = fl(acc * sc + sh), |acc - y| <= b,
  fused or not:
    not fused  fl(fl(acc sc) + sh): the product within u |acc sc|, the sum within u (|acc sc| (1 + u) + |sh|);
    fused      one rounding of acc sc + sh, within u (|acc sc| + |sh|);
  and |acc sc| <= |sc| (|y| + b), so
    bz = |sc| b + 2 u (|sc y| + |sh|)  +  2 u |sc| b (1 + u) + u^2 |sc y|,
  the last two being the second-order remainder of the same expansion, charged as (1 + 3 u) on the first-order terms.
  sc, sh broadcast against y (NCHW: pass them as [1, C, 1, 1])."""
  y, b, sc, sh = (torch.as_tensor(t, dtype=torch.float64) for t in (y, b, sc, sh))
  z = sc * y + sh
  bz = (sc.abs() * b + 2 * U32 * ((sc * y).abs() + sh.abs())) * (1 + 3 * U32)
  return z, bz


def pool_s2p1(a):
  """2x2 / stride 2 / padding 1 max-pool of NCHW values >= 0 (post-ReLU: the padding is as good as zero)."""
  return torch.nn.functional.max_pool2d(a, 2, 2, padding=1)


def pooled_bracket(y, b, sc, sh):
  """z, bz, lo, hi of bf16_rne(pool(relu(fl(acc sc + sh)))) for |acc - y| <= b.

  ReLU, max and round-to-nearest-even are non-decreasing, and so is their composition in either order (the stem stores
  f32_to_bf16(fmaxf(z, 0)) per pixel and takes the 2x2 max of the bf16 values: csrc/stem.hip stem_apply_pool_kernel --
  rne(max) = max(rne)).  With the fp32 z within bz of the float64 z (affine_bound) the stored value lies in
    [bf16_rne(pool(relu(z - bz))), bf16_rne(pool(relu(z + bz)))];
  lo <= got <= hi is the whole assertion."""
  z, bz = affine_bound(y, b, sc, sh)
  lo = bf16_rne(pool_s2p1(torch.relu(z - bz)))
  hi = bf16_rne(pool_s2p1(torch.relu(z + bz)))
  return z, bz, lo, hi


def bf16_half_spacing(v, err=0.0):
  """Largest |bf16_rne(t) - t| over |t| <= |v| + err: half the bf16 spacing at |v| + err (the spacing does not decrease
  with the magnitude).  This, not U16 / 2 relative, is what a round-to-nearest store costs: just above a power of two
  half a spacing is 2^-8 |t|, just below the next one 2^-9 |t|."""
  v = torch.as_tensor(v, dtype=torch.float64)
  return 0.5 * bf16_spacing(v.abs() + err)


# ----------------------------------------------------------------------------------------------------------------------
# IID losses (csrc/iid_loss.hip, csrc/seg_loss.hip): the float64 k x k stage and the bf16 three-term split of the
# segmentation joint (tests/iid_stage_cases.py, tests/test_iid_stages_cpu.py, tests/test_gpu_iid_stages.py)
# ----------------------------------------------------------------------------------------------------------------------
U64 = 2.0 ** -53


def stage_n(k, nparts):
  """Float64 roundings on the longest path from the fp32 partials to an output of the k x k stage, counted in the
  kernels' code.  iid_loss_kernel (k < 96), an entry of dR:
    nparts       the partial sums a, b (nparts - 1 additions each, they are parallel) and a + b; the 0.5 is exact
    k k - 1      S: per-thread chain, six wave_sum_d steps, the fold of the per-wave values in block_sum_d -- a tree over
                 k k leaves however it is grouped (additions of a zero padding lane are exact)
    2            invS = 1 / S and P = Ps invS
    k - 1        the marginal p_i (row sum of P: per-lane chain and wave_sum_d); the clamped row sum runs in parallel
    1            log of the clamped marginal (charged as one rounding, as for every other operation)
    10           the entry's d: lamb lj, lP - ., lamb li, - ., - 1, s_rc / p_i, rowi + colj, lamb (.), + ., and log Pc
                 in parallel with log p_i (one of the two is on the path; both are charged: 10)
    k k          g = sum d P: one product per term and a tree over k k leaves
    2            (d - g) invS
  n = nparts + 2 k k + k + 13.  The scalars stop after the sum of the k k loss terms (no `(d - g) invS`): fewer.
  The four iid_big_* kernels (k >= 96) compute the same expressions: S and the four block sums are a per-thread chain,
  wave_sum_d, block_sum_d and a fold over the 32 blocks in index order -- again trees over k k leaves -- and the per-row
  logarithm and row term are computed once per row instead of per entry, which removes roundings from no path and adds
  none.  Same count; n is the larger of the two because they are equal."""
  return nparts + 2 * k * k + k + 13


def stage_bound(ref, mag, k, nparts):
  """|got - ref| for an fp32 output of the k x k stage: ONE fp32 rounding of a float64 computation,
      U32 |ref| + 2 n u64 / (1 - 2 n u64) mag,   u64 = 2^-53, n = stage_n(k, nparts).
  mag: sum of the magnitudes of the terms the output is made of, from the float64 reference (for the two scalars
  M = sum Pc (|log Pc| + lamb |log p_i| + lamb |log p_j|); for an entry of dR the magnitudes of d's terms plus those of
  g's, over S) -- a computed value is its exact value times a product of at most n factors (1 + e), |e| <= u64, hence
  within n u64 / (1 - n u64) of it relative to the magnitudes (Higham, lemma 3.1).  The factor 2: the float64 reference
  this is compared with performs the same operations in float64 (torch's sums in another grouping, of at most the same
  depth) and so carries an error of the same form itself -- n for the kernel, n for the reference.  The fp32 store
  rounds to nearest: half a spacing, which just above a power of two is U32 = 2^-24 of the value -- the first term is
  attained (measured worst |err| / bound 0.997), so the bound has no room for a second fp32 rounding anywhere.
  Not covered by the form above, stated rather than hidden: a relative error e in the ARGUMENT of a logarithm is an
  absolute error e in its value, which mag charges as e |log|; where |log| < 1 (a marginal above 1 / e: k <= 2) that
  undercounts by at most a factor 1 / |log|, against a count n that charges the k k-term sums at their worst case."""
  n = 2 * stage_n(k, nparts)
  assert n * U64 < 1
  ref, mag = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(mag, dtype=torch.float64)
  return U32 * ref.abs() + (n * U64 / (1.0 - n * U64)) * mag


# seg_split8 (csrc/seg_loss.hip): x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), each rounded to
# nearest even, the subtractions exact in fp32.  bf16 has 8 significant bits: for 2^e <= |x| < 2^(e+1) its spacing is
# 2^(e-7), so |x - h| <= 2^(e-8) <= 2^-8 |x| -- NOT 2^-9 |x|, which holds only in the upper half of a binade -- hence
# |m| <= 2^-8 |x|, |x - h - m| <= 2^-8 |x - h| <= 2^-16 |x| and |l| <= 2^-16 |x|.  x - h lies on x's grid 2^(e-23) below
# 2^(e-8) (16 bits), x - h - m on the same grid at or below 2^(e-16): at most 8 bits, so l holds it exactly and
# x = h + m + l with no remainder (tests/test_iid_stages_cpu.py checks all three on every draw; no underflow: the
# operands are floored at 2^-60).
# The product x x' = (h + m + l)(h' + m' + l') has nine terms; seg_mfma6 keeps h h', h m', m h', h l', l h', m m' and
# drops m l', l m', l l':  |dropped| <= (2 . 2^-8 2^-16 + 2^-32) |x x'| = (2^-23 + 2^-32) |x x'|.
# The kernel's comment claimed "below 2^-24 of the product".  That is the typical size (m and l are spread over their
# ranges and enter with both signs), not a bound: the worst case is twice that, and the bound below charges it.
SPLIT_D = 2.0 ** -23 + 2.0 ** -32
# sum of the magnitudes of the six kept products <= (|h| + |m| + |l|)(|h'| + |m'| + |l'|)
#   <= (1 + 2^-8 + 2^-8 + 2^-16)^2 |x x'| < (1 + 2^-5) |x x'|
SPLIT_KEPT = 1.0 + 2.0 ** -5


def split_joint_bound(terms, A):
  """|sum of fp32 partials - exact joint entry| for seg_joint_bf16_kernel: the six kept products of every pixel product
  are exact in fp32 (8 x 8 bits) and accumulated in fp32 -- fma_acc_bound over 6 `terms` leaves whose magnitudes sum to
  at most SPLIT_KEPT A -- plus the dropped products, SPLIT_D A.  A: the contraction on the magnitudes, float64."""
  return fma_acc_bound_each(6 * torch.as_tensor(terms, dtype=torch.float64), SPLIT_KEPT * A) + SPLIT_D * A


def fma_acc_bound_each(terms, A):
  """fma_acc_bound with a term count per element (`terms` a tensor that broadcasts against A): the shifts of the
  segmentation joint overlap in different numbers of pixels."""
  n = torch.as_tensor(terms, dtype=torch.float64) + 1
  assert float(n.max()) * U32 < 1
  return (n * U32 / (1.0 - n * U32)) * A
