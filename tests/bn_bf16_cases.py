"""Inputs, float64 references and derived bounds for the bf16 BatchNorm kernels of csrc/bn.hip, written once and used
twice: tests/test_gpu_bn_bf16.py runs them against the C entry points on the GPU, tests/test_bn_bf16_cpu.py against a
numpy emulation of the kernels (to prove that the bounds admit the correct arithmetic, fused or not, and reject seeded
defects).  A "backend" is an object with apply / reduce / bwd_apply / finalize / bwd_finalize that takes and returns
CPU tensors (interiors only, [N, H, W, C] float32 holding bf16 values).

Every bound is a formula of U32 = 2^-24 (one fp32 operation), U16 = 2^-8 (one bf16 store), EPS64 = 2^-53 (one float64
operation of the finalisers), magnitudes of the terms and counts."""
import functools

import numpy as np
import torch

from tests.parity import U16, U32, _mask_act, _masked_g, _pow2_coef, assert_within, rnd

EPS64 = 2.0 ** -53
BN_EPS = float(np.float32(1e-5))
MOMENTUM = float(np.float32(0.1))

# (N, H, W, P, C), one hazard each (see the docstring of tests/test_gpu_bn_bf16.py)
SHAPES = [(6, 13, 13, 1, 128), (1, 1, 1, 1, 64), (3, 3, 5, 2, 64), (2, 20, 36, 2, 64), (5, 49, 49, 1, 64),
          (11, 7, 7, 1, 512), (3, 5, 3, 1, 1024), (2, 3, 5, 1, 2048)]
# channel counts check_c refuses: the first-generation kernels, and no reduction at all
FIRST_GEN_SHAPES = [(2, 5, 7, 1, 8), (2, 5, 7, 1, 24), (2, 5, 7, 1, 192)]


def bf16(t):
  return t.to(torch.bfloat16).float()


def check_c(C):
  """bn.hip check_c: the channel counts the pixel walkers and the reduction take."""
  return C % 64 == 0 and 256 % (C // 8) == 0 and C <= 2048


def v2_grid(npx, C, reduce):
  """bn.hip bn_v2_grid restated: (pixels per block, blocks, pixel lanes)."""
  PL = 256 // (C >> 3)
  blocks = 1024
  if reduce:
    blocks = 512 if C <= 128 else 256
  p = (npx + blocks - 1) // blocks
  p = (p + 2 * PL - 1) // (2 * PL) * (2 * PL)
  return p, (npx + p - 1) // p, PL


@functools.lru_cache(maxsize=None)
def inputs(N, H, W, P, C):
  """bf16-rounded tensors and fp32 coefficients of one shape (shared, never modified).  y lies on multiples of 1/8 and
  the mask coefficients on small dyadics: the mask expression is exact in fp32, fused or not."""
  rng = np.random.default_rng(N * 7 + C + 131 * H + W)
  y = torch.round(rnd(rng, N, H, W, C) * 8) / 8
  assert torch.equal(bf16(y), y)
  d = dict(y=y, y2=bf16(rnd(rng, N, H, W, C)), res=bf16(rnd(rng, N, H, W, C)), dout=bf16(rnd(rng, N, H, W, C)),
           act=bf16(_mask_act(rng, N, H, W, C)), coef=rnd(rng, 5, C), coef2=rnd(rng, 5, C),
           mcoef=torch.cat([_pow2_coef(rng, C), torch.zeros(3, C)]), b1=rnd(rng, 3, C), b2=rnd(rng, 3, C))
  d["b1"][1, 0::4] = 0.0        # c2 = 0: where g = 0 as well the output is the stored c3, exactly
  d["b2"][1, 1::4] = 0.0
  return d


# --------------------------------------------------------------------------------------
# (a) bn_apply
# --------------------------------------------------------------------------------------
APPLY_COMBOS = [(relu, use_res, use_y2) for relu in (0, 1) for use_res in (False, True) for use_y2 in (False, True)]


def apply_reference(y, coef, res, y2, coef2, relu):
  """float64 out and A, the sum of the magnitudes of the terms."""
  c = coef.double()
  v = y.double() * c[0] + c[1]
  A = (y.double() * c[0]).abs() + c[1].abs()
  if res is not None:
    v, A = v + res.double(), A + res.double().abs()
  if y2 is not None:
    c2 = coef2.double()
    v, A = v + y2.double() * c2[0] + c2[1], A + (y2.double() * c2[0]).abs() + c2[1].abs()
  return (v.clamp_min(0) if relu else v), A


def check_apply_with(be, shape, y, coef, res, y2, coef2, relu, what):
  """out = [relu](y*scale + shift [+ res] [+ y2*scale2 + shift2]): at most six fp32 operations, each within U32 of a
  partial result that A bounds, then one bf16 store: 6 * U32 * A + U16 * |ref|."""
  out = be.apply(y, coef, res, y2, coef2, relu, shape)
  ref, A = apply_reference(y, coef, res, y2, coef2, relu)
  assert_within(out, ref, 6 * U32 * A + U16 * ref.abs(), what, family="bn_apply")


def check_apply(be, shape):
  i = inputs(*shape)
  for relu, use_res, use_y2 in APPLY_COMBOS:
    check_apply_with(be, shape, i["y"], i["coef"], i["res"] if use_res else None, i["y2"] if use_y2 else None,
                     i["coef2"] if use_y2 else None, relu, "bn_apply %s relu=%d res=%d y2=%d" % (shape, relu, use_res, use_y2))


# --------------------------------------------------------------------------------------
# (b) bn_bwd_reduce
# --------------------------------------------------------------------------------------
MASK_MODES = ("none", "act", "mask_coef")


def keep_fraction(i, mode):
  if mode == "act":
    return float((i["act"] > 0).float().mean())
  return float((i["y"] * i["mcoef"][0] + i["mcoef"][1] > 0).float().mean())


def check_reduce(be, shape):
  """sums = (sum g, sum g*y) [sums2 = (sum g, sum g*y2)] against the float64 sums of the exact products.  The
  accumulators add the blocks' fp32 partials exactly, so the only error is the fp32 summation of one block's pixels:
  n_block * U32 * sum |terms| per channel, n_block = the pixels of the largest chunk (v2_grid)."""
  N, H, W, P, C = shape
  i = inputs(*shape)
  n_block = v2_grid(N * H * W, C, 1)[0]
  for mode in MASK_MODES:
    if mode != "none":
      assert 0.2 < keep_fraction(i, mode) < 0.8, (mode, keep_fraction(i, mode))
    for use_y2 in (False, True):
      s1, s2 = be.reduce(i["dout"], i["act"] if mode == "act" else None, i["y"], i["y2"] if use_y2 else None,
                         i["mcoef"] if mode == "mask_coef" else None, shape)
      g = _masked_g(i["dout"], i["act"], i["y"], i["mcoef"], mode).double()
      for st, yy in ((s1, i["y"]),) + (((s2, i["y2"]),) if use_y2 else ()):
        terms = torch.stack([g, g * yy.double()])
        assert_within(st, terms.sum((1, 2, 3)), n_block * U32 * terms.abs().sum((1, 2, 3)),
                      "bn_bwd_reduce %s mask=%s y2=%d" % (shape, mode, use_y2), family="bn_bwd_reduce")
      if use_y2:
        assert torch.equal(s2[0], s1[0]), "sums2[0] != sums[0]"
      else:
        assert s2 is None


# --------------------------------------------------------------------------------------
# (c) bn_bwd_apply
# --------------------------------------------------------------------------------------
def check_bwd_apply(be, shape, modes=MASK_MODES, gen2=False):
  """dy = c1*g + c2*y + c3 (dy2 from y2 with its own coefficients): four fp32 operations within U32 of a partial result
  bounded by A = |c1 g| + |c2 y| + |c3|, one bf16 store: 4 * U32 * A + U16 * |ref|; where g = 0 and c2 = 0 every
  product is an exact zero and the output is the stored c3."""
  i = inputs(*shape)
  for mode in modes:
    for use_y2 in (False, True):
      dy, dy2 = be.bwd_apply(i["dout"], i["act"] if mode == "act" else None, i["y"], i["b1"], i["y2"] if use_y2 else None,
                             i["b2"] if use_y2 else None, i["mcoef"] if mode == "mask_coef" else None, shape, gen2)
      g = _masked_g(i["dout"], i["act"], i["y"], i["mcoef"], mode).double()
      for out, yy, b in ((dy, i["y"], i["b1"]),) + (((dy2, i["y2"], i["b2"]),) if use_y2 else ()):
        what = "bn_bwd_apply %s mask=%s y2=%d" % (shape, mode, use_y2)
        bd = b.double()
        ref = bd[0] * g + bd[1] * yy.double() + bd[2]
        A = (bd[0] * g).abs() + (bd[1] * yy.double()).abs() + bd[2].abs()
        assert_within(out, ref, 4 * U32 * A + U16 * ref.abs(), what, family="bn_bwd_apply")
        exact = (g == 0) & (b[1] == 0)
        if mode != "none":
          assert bool(exact.any()), "no element with g = 0 and c2 = 0"
        assert torch.equal(out[exact], bf16(b[2]).expand_as(out)[exact]), what + ": not the stored c3 where g = 0 and c2 = 0"
      if not use_y2:
        assert dy2 is None


# --------------------------------------------------------------------------------------
# (d) the finalisers
# --------------------------------------------------------------------------------------
FIN_C = 64
FIN_FAMILIES = ("ordinary", "mean100", "constant", "clamp")       # channel c belongs to family c % 4
FIN_COUNTS = [(48, 0), (1, 0), (48, 96), (2304, 0)]                # (count, unbiased_count; 0 = the same)


@functools.lru_cache(maxsize=None)
def finalize_inputs(count):
  """fp32 sums [2, C] of `count` values per channel, by family, plus parameters and running statistics."""
  rng = np.random.default_rng(count)
  s, ss = np.zeros(FIN_C), np.zeros(FIN_C)
  for c in range(FIN_C):
    fam = FIN_FAMILIES[c % 4]
    if fam == "ordinary":
      v = rng.standard_normal(count) * 1.5 + 0.3
      s[c], ss[c] = v.sum(), (v * v).sum()
    elif fam == "mean100":                   # half at 100.5: variance 1/16 under a mean near 100
      v = np.where(np.arange(count) < count // 2, 100.5, 100.0)
      s[c], ss[c] = v.sum(), (v * v).sum()
    elif fam == "constant":                  # sums exact in fp32: the variance is exactly 0
      s[c], ss[c] = count * 1.5, count * 2.25
    else:                                    # a constant whose rounded sums give ss/count - m^2 < 0
      while True:
        x = float(np.float32(rng.uniform(0.5, 3.0)))
        s[c], ss[c] = count * x, count * x * x
        if float(np.float32(ss[c])) / count - (float(np.float32(s[c])) / count) ** 2 < 0:
          break
  sums = torch.from_numpy(np.stack([s, ss])).float()
  gamma, beta = 1 + 0.2 * rnd(rng, FIN_C), 0.1 * rnd(rng, FIN_C)
  return sums, gamma, beta, rnd(rng, FIN_C), rnd(rng, FIN_C).abs() + 0.5


def invstd_bound(v, dv):
  """invstd = rsqrtf(var + eps): one U32 for rounding var + eps, one for rsqrtf (bn.hip: about 1 ulp), one for the
  store, all relative to invstd, plus the error dv of var through d/dv (v + eps)^-1/2 = -invstd / (2 (v + eps))."""
  inv = 1.0 / torch.sqrt(v + BN_EPS)
  return inv, 3 * U32 * inv + 0.5 * inv / (v + BN_EPS) * dv


def scale_shift_bounds(gamma, beta, m, tol_m, inv, tol_inv):
  """scale = gamma * invstd (one operation), shift = beta - mean * scale (two)."""
  sc = gamma * inv
  tol_sc = gamma.abs() * tol_inv + U32 * sc.abs()
  sh = beta - m * sc
  tol_sh = m.abs() * tol_sc + sc.abs() * tol_m + 2 * U32 * (beta.abs() + (m * sc).abs())
  return sc, tol_sc, sh, tol_sh


def check_finalize(be, count, ucount):
  """iic_bn_finalize(training=1) per channel against float64 on the fp32 sums that were encoded."""
  sums, gamma, beta, rm0, rv0 = finalize_inputs(count)
  coef, rm, rv, nbt = be.finalize(sums, gamma, beta, rm0, rv0, 3, count, ucount, 1)
  what = "bn_finalize count=%d ucount=%d: " % (count, ucount)
  assert nbt == 4, "num_batches_tracked did not advance by 1"
  s, ss, g64, b64 = sums[0].double(), sums[1].double(), gamma.double(), beta.double()
  m, q = s / count, ss / count
  raw = q - m * m
  fam = torch.arange(FIN_C) % 4
  assert bool((raw[fam == 3] < 0).all()) and bool((raw[fam == 2] == 0).all())
  v = raw.clamp_min(0)
  canc = 4 * EPS64 * (q + m * m)                    # float64 cancellation in ss/count - m^2, kernel and reference
  tol_m = U32 * m.abs()
  assert_within(coef[2], m, tol_m, what + "mean", family="bn_finalize mean")
  u = ucount if ucount > 0 else count
  f = u / (u - 1.0) if u > 1 else 1.0
  unb = v * f
  assert_within(coef[4], unb, U32 * unb + f * canc + 2 * EPS64 * unb, what + "unbiased variance", family="bn_finalize var")
  inv, tol_inv = invstd_bound(v, U32 * v + canc)
  assert bool(torch.isfinite(coef).all())
  assert_within(coef[3], inv, tol_inv, what + "invstd", family="bn_finalize invstd")
  assert_within(coef[3][fam == 2], torch.full((FIN_C // 4,), BN_EPS, dtype=torch.float64).rsqrt(), 3 * U32 * inv[fam == 2],
                what + "invstd of a constant channel", family="bn_finalize invstd")
  sc, tol_sc, sh, tol_sh = scale_shift_bounds(g64, b64, m, tol_m, inv, tol_inv)
  assert_within(coef[0], sc, tol_sc, what + "scale", family="bn_finalize scale/shift")
  assert_within(coef[1], sh, tol_sh, what + "shift", family="bn_finalize scale/shift")
  # running statistics from the kernel's own fp32 mean / unbiased variance: r' = (1 - m) r + m s, four operations
  for got, r0, new in ((rm, rm0, coef[2]), (rv, rv0, coef[4])):
    r0, new = r0.double(), new.double()
    assert_within(got, (1 - MOMENTUM) * r0 + MOMENTUM * new, 4 * U32 * (r0.abs() + new.abs()), what + "running statistics",
                  family="bn_finalize running")
  rel = ((coef[3].double() - inv).abs() / inv)
  return float((rel / U32).max())                    # measured invstd error, in units of U32, for the record


def check_finalize_eval(be):
  """iic_bn_finalize(training=0): mean and var are the running statistics themselves; nothing else changes."""
  sums, gamma, beta, rm0, rv0 = finalize_inputs(48)
  coef, rm, rv, nbt = be.finalize(None, gamma, beta, rm0, rv0, 3, 48, 0, 0)
  assert nbt == 3 and torch.equal(rm, rm0) and torch.equal(rv, rv0)
  assert torch.equal(coef[2], rm0)
  m, v = rm0.double(), rv0.double()
  inv, tol_inv = invstd_bound(v, torch.zeros_like(v))
  assert_within(coef[3], inv, tol_inv, "eval invstd", family="bn_finalize invstd")
  sc, tol_sc, sh, tol_sh = scale_shift_bounds(gamma.double(), beta.double(), m, torch.zeros_like(m), inv, tol_inv)
  assert_within(coef[0], sc, tol_sc, "eval scale", family="bn_finalize scale/shift")
  assert_within(coef[1], sh, tol_sh, "eval shift", family="bn_finalize scale/shift")
  return coef


@functools.lru_cache(maxsize=None)
def bwd_finalize_inputs():
  """fp32 (s, sy), mean, invstd, gamma.  Odd channels: sy within a few ulps of mean*s (cancellation in sgx)."""
  rng = np.random.default_rng(17)
  C = FIN_C
  s, mean = rnd(rng, C) * 20, rnd(rng, C) * 2 + 0.5
  sy = rnd(rng, C) * 30
  near = (mean.double() * s.double()).float()
  near = torch.from_numpy(np.nextafter(near.numpy(), np.float32(np.inf) * np.sign(rnd(rng, C).numpy())))
  sy[1::2] = near[1::2]
  sy[3::8] = (mean.double() * s.double()).float()[3::8]
  return torch.stack([s, sy]), mean, rnd(rng, C).abs() + 0.3, 1 + 0.2 * rnd(rng, C)


def check_bwd_finalize(be, count=507):
  """c1, c2, dgamma, dbeta within U32 * |ref| of the float64 formula on the same fp32 inputs (one rounding of a float64
  value; the kernel's own float64 operations, at most eight in a chain, add 8 * EPS64 of the magnitudes), c3 within
  U32 * (|c1 s / count| + |c2 mean|)."""
  sums, mean, invstd, gamma = bwd_finalize_inputs()
  bcoef, dgamma, dbeta = be.bwd_finalize(sums, gamma, mean, invstd, count)
  s, sy, mu, inv, g = sums[0].double(), sums[1].double(), mean.double(), invstd.double(), gamma.double()
  sgx = (sy - mu * s) * inv
  c1 = g * inv
  c2 = -c1 * sgx * inv / count
  c3 = -c1 * s / count - c2 * mu
  mag3 = (c1 * s / count).abs() + (c2 * mu).abs()
  for got, ref, mag, what in ((bcoef[0], c1, c1.abs(), "c1"), (bcoef[1], c2, c2.abs(), "c2"), (bcoef[2], c3, mag3, "c3"),
                              (dgamma, sgx, sgx.abs(), "dgamma"), (dbeta, s, s.abs(), "dbeta")):
    assert_within(got, ref, (U32 + 8 * EPS64) * mag, "bn_bwd_finalize " + what, family="bn_bwd_finalize")


# --------------------------------------------------------------------------------------
# (f) data on the ReLU boundary
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boundary_inputs(N, H, W, P, C):
  """y [N, H, W, C] (bf16 values), coef [5, C] and the share of elements on which the unfused fp32 predicate
  fl32(fl32(scale*y) + shift) > 0 differs from the exact sign of scale*y + shift.  Per channel: a random (non-dyadic)
  fp32 scale, one bf16 value y0 and shift = -fl32(scale*y0); about a quarter of the pixels hold y0, another quarter its
  two bf16 neighbours, the rest random values.  At y0 the exact expression is the rounding residual of scale*y0: y0 is
  drawn again (a few times, and not for every fourth channel) until that residual is positive, so that both signs occur
  and the positive one -- where the two predicates differ -- on well over 10 % of the elements."""
  rng = np.random.default_rng(C * 3 + N)
  scale = rnd(rng, C)
  scale = torch.where(scale.abs() < 0.05, torch.full_like(scale, 0.7310585), scale)
  y0 = torch.zeros(C)
  for c in range(C):
    for _ in range(8):
      y0[c] = float(bf16(torch.tensor(float(rng.standard_normal()) * 1.5 + 0.1)))
      resid = float(scale[c].double() * y0[c].double() - (scale[c] * y0[c]).double())
      if y0[c] != 0 and (resid > 0 or c % 4 == 0):
        break
  shift = -(scale * y0)                                              # fp32 product
  up = (y0.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16).float()
  down = (y0.to(torch.bfloat16).view(torch.int16) - 1).view(torch.bfloat16).float()
  r = torch.from_numpy(rng.random((N, H, W, C)))
  y = bf16(rnd(rng, N, H, W, C))
  y = torch.where(r < 0.25, y0.expand_as(y), y)
  y = torch.where((r >= 0.25) & (r < 0.375), up.expand_as(y), y)
  y = torch.where((r >= 0.375) & (r < 0.5), down.expand_as(y), y)
  unfused = (y * scale + shift) > 0                                  # two fp32 operations
  exact = (y.double() * scale.double() + shift.double()) > 0
  coef = torch.cat([torch.stack([scale, shift]), torch.zeros(3, C)])
  return y, coef, float((unfused != exact).float().mean())
