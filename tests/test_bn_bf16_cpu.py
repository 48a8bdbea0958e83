"""CPU proof of the bounds of tests/test_gpu_bn_bf16.py: they must admit the correct kernel and reject real defects.

The kernels of csrc/bn.hip are emulated in numpy: fp32 operations, the multiply-adds once fused (a*b exact, one
rounding; evaluated in float64, where the product of two fp32 values is exact, and rounded to fp32 -- a fused
multiply-add up to a double rounding that is far below every bound) and once unfused, round-to-nearest-even bf16
stores, the chunked reduction with fp32 per-block partials and the pixel walker (bn_v2_grid, px_start, px_advance
restated here and checked against plain enumeration).  Every check of tests/bn_bf16_cases.py that the GPU file runs on
the C entry points runs here on both emulations, on the same inputs; then one-term defects are seeded into the emulation
and the same checks must fail.  For each defect the docstring says whether the criterion of
test_bn_forward_backward_kernels (one shape, 2e-2 absolute, 1e-2 * max, rtol 2e-3) would have failed as well; that is
computed by _old_criterion_rejects and asserted, not guessed."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import bn_bf16_cases as cases
from tests.parity import SENTINEL

f32, f64 = np.float32, np.float64


def _np(t):
  return None if t is None else t.numpy().astype(f32)


def _bf16(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).float().numpy()


def mad(a, b, c, fused):
  """fl32(a*b + c), fused or as two fp32 operations."""
  if fused:
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
  return (a * b + c).astype(f32)             # numpy rounds every fp32 operation


# --------------------------------------------------------------------------------------
# the pixel walker of the second-generation kernels, offsets in pixels (the kernel's offset / C, without c8 * 8)
# --------------------------------------------------------------------------------------
def px_start(q, H, W, P):
  row = q // W
  x = q - row * W
  n = row // H
  yy = row - n * H
  return [x, yy, (n * (H + 2 * P) + yy + P) * (W + 2 * P) + P + x]


def px_advance(w, step, H, W, P, skip=2):
  w[0] += step
  w[2] += step
  while w[0] >= W:
    w[0] -= W
    w[2] += skip * P                         # right + left border (a defect writes skip = 1)
    w[1] += 1
    if w[1] == H:
      w[1] = 0
      w[2] += 2 * P * (W + 2 * P)


def walk(shape, reduce, drop_tail=False, skip=2):
  """Padded pixel offsets [blocks, PL, steps] in the order thread (block, pl) visits them, -1 where it has none: the
  loops of bn_bwd_reduce2_kernel / bn_bwd_apply2_kernel (pair loop, then the tail)."""
  N, H, W, P, C = shape
  npx = N * H * W
  per, grid, PL = cases.v2_grid(npx, C, reduce)
  out = -np.ones((grid, PL, per // PL), dtype=np.int64)
  for b in range(grid):
    q0, q1 = b * per, min(b * per + per, npx)
    for pl in range(PL):
      if q0 + pl >= q1:
        continue
      wa, q, k = px_start(q0 + pl, H, W, P), q0 + pl, 0
      while q + PL < q1:
        wb = list(wa)
        px_advance(wb, PL, H, W, P, skip)
        out[b, pl, k], out[b, pl, k + 1] = wa[2], wb[2]
        wa = list(wb)
        px_advance(wa, PL, H, W, P, skip)
        q, k = q + 2 * PL, k + 2
      if q < q1 and not drop_tail:
        out[b, pl, k] = wa[2]
  return out


def interior_offsets(shape):
  N, H, W, P, C = shape
  n, yy, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
  return ((n * (H + 2 * P) + yy + P) * (W + 2 * P) + P + x).reshape(-1)


@pytest.mark.parametrize("reduce", [0, 1])
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_walker_visits_every_interior_pixel_once_in_order(shape, reduce):
  """Thread (block, pl) must visit the pixels q0 + pl, q0 + pl + PL, ... of its chunk: against plain enumeration."""
  N, H, W, P, C = shape
  per, grid, PL = cases.v2_grid(N * H * W, C, reduce)
  assert per % (2 * PL) == 0 and (grid - 1) * per < N * H * W <= grid * per
  want, got = interior_offsets(shape), walk(shape, reduce)
  for b in range(grid):
    for pl in range(PL):
      mine = want[b * per:(b + 1) * per][pl::PL]
      assert list(got[b, pl, :len(mine)]) == list(mine) and bool((got[b, pl, len(mine):] == -1).all()), (b, pl)


def test_grid_restatement_matches_the_shapes_hazards():
  """The chunking the shapes were chosen for (bn_v2_grid with reduce = 1)."""
  g = lambda s: cases.v2_grid(s[0] * s[1] * s[2], s[4], 1)
  assert g((5, 49, 49, 1, 64)) == (64, 188, 32) and 12005 - 187 * 64 == 37
  assert g((11, 7, 7, 1, 512)) == (8, 68, 4) and 539 - 67 * 8 == 3
  assert g((3, 5, 3, 1, 1024))[2] == 2 and g((2, 3, 5, 1, 2048))[2] == 1
  assert g((3, 3, 5, 2, 64))[2] == 32 > 15
  assert all(not cases.check_c(s[4]) for s in cases.FIRST_GEN_SHAPES) and all(cases.check_c(s[4]) for s in cases.SHAPES)


# --------------------------------------------------------------------------------------
# the kernels
# --------------------------------------------------------------------------------------
def _pad(x, P, fill=0.0):
  N, H, W, C = x.shape
  out = np.full((N, H + 2 * P, W + 2 * P, C), fill, dtype=f32)
  out[:, P:P + H, P:P + W] = x
  return out.reshape(-1, C)


class Emu:
  """numpy emulation of bn.hip as a backend of tests/bn_bf16_cases.py.  defect: None or one of DEFECTS."""

  def __init__(self, fused, defect=None):
    self.fused, self.defect = fused, defect

  def _coef(self, c):
    c = _np(c)
    return np.roll(c, -8, axis=1) if self.defect == "coef_plus8" else c       # channel c reads c + 8

  def _keep(self, act, y, mcoef):
    if act is not None:
      return act >= 0 if self.defect == "mask_ge" else act > 0
    m = mad(y, mcoef[0], mcoef[1], self.fused)
    return m >= 0 if self.defect in ("mask_ge", "mask_ge_coef") else m > 0

  def apply(self, y, coef, res, y2, coef2, relu, shape):
    c = self._coef(coef)
    v = mad(_np(y), c[0], c[1], self.fused)
    if res is not None:
      v = v + _np(res)
    if y2 is not None:
      c2 = self._coef(coef2)
      sh2 = np.zeros_like(c2[1]) if self.defect == "shift2_omitted" else c2[1]
      v = v + mad(_np(y2), c2[0], sh2, self.fused)
    if relu:
      v = np.maximum(v, f32(0))
    return torch.from_numpy(_bf16(v))

  def _walk(self, shape, reduce):
    return walk(shape, reduce, drop_tail=self.defect == "tail_dropped", skip=1 if self.defect == "border_skip" else 2)

  def reduce(self, dout, act, y, y2, mcoef, shape):
    N, H, W, P, C = shape
    G, Y = _pad(_np(dout), P), _pad(_np(y), P)
    if act is not None or mcoef is not None:
      keep = self._keep(None if act is None else _pad(_np(act), P), Y, None if mcoef is None else _np(mcoef))
      G = np.where(keep, G, f32(0))
    Y2 = None if y2 is None else _pad(_np(y2), P)
    idx = self._walk(shape, 1)
    grid, PL, steps = idx.shape
    sg, sgy, sgy2 = (np.zeros((grid, PL, C), dtype=f32) for _ in range(3))
    for k in range(steps):
      valid = (idx[:, :, k] >= 0)[..., None]
      at = np.maximum(idx[:, :, k], 0)
      g = np.where(valid, G[at], f32(0))
      sg = sg + g
      sgy = mad(g, np.where(valid, Y[at], f32(0)), sgy, self.fused)
      if Y2 is not None:
        sgy2 = mad(g, np.where(valid, Y2[at], f32(0)), sgy2, self.fused)

    def fold(s):                                     # LDS reduction over the pixel lanes, then the exact cells
      t = np.zeros((grid, C), dtype=f32)
      for p in range(PL):
        t = t + s[:, p]
      return t.astype(f64).sum(0)
    s1 = torch.from_numpy(np.stack([fold(sg), fold(sgy)]))
    return s1, (torch.from_numpy(np.stack([fold(sg), fold(sgy2)])) if Y2 is not None else None)

  def bwd_apply(self, dout, act, y, b1, y2, b2, mcoef, shape, gen2):
    N, H, W, P, C = shape
    G, Y = _pad(_np(dout), P), _pad(_np(y), P)
    if act is not None or mcoef is not None:
      keep = self._keep(None if act is None else _pad(_np(act), P), Y, None if mcoef is None else _np(mcoef))
      G = np.where(keep, G, f32(0))
    if cases.check_c(C) and (gen2 or act is None):     # the pixel walker; otherwise the first generation
      at = self._walk(shape, 0).reshape(-1)
      at = at[at >= 0]
    else:
      at = interior_offsets(shape)
    outs = []
    for yy, b in ((Y, b1),) + (((_pad(_np(y2), P), b2),) if y2 is not None else ()):
      k = self._coef(b)
      if self.fused:
        o = (mad(k[1], yy[at], k[0] * G[at], True) + k[2]).astype(f32)
      else:
        o = ((k[0] * G[at] + k[1] * yy[at]) + k[2]).astype(f32)
      out = np.full_like(Y, SENTINEL)
      out[at] = _bf16(o)
      out = out.reshape(N, H + 2 * P, W + 2 * P, C)
      border = np.ones(out.shape[1:3], dtype=bool)
      border[P:P + H, P:P + W] = False
      assert bool((out[:, border] == SENTINEL).all()), "the PT border was written"
      outs.append(torch.from_numpy(out[:, P:P + H, P:P + W].copy()))
    return outs[0], (outs[1] if y2 is not None else None)

  def finalize(self, sums, gamma, beta, rm0, rv0, nbt0, count, ucount, training):
    C = gamma.shape[0]
    gamma, beta, rm, rv = _np(gamma), _np(beta), _np(rm0).copy(), _np(rv0).copy()
    eps, mom = f32(cases.BN_EPS), f32(cases.MOMENTUM)
    unbf = np.zeros(C, dtype=f32)
    if training:
      s, ss = sums[0].numpy().astype(f64), sums[1].numpy().astype(f64)
      m, q = s / count, ss / count
      if self.fused:     # ss/count - m*m as one fused float64 operation
        v = np.array([float(Fraction(float(a)) - Fraction(float(b)) ** 2) for a, b in zip(q, m)])
      else:
        v = q - m * m
      v = np.maximum(v, 0.0)
      u = ucount if ucount > 0 else count
      unb = v * float(u) / float(u - 1) if u > 1 else v
      mean, var, unbf = m.astype(f32), v.astype(f32), unb.astype(f32)
      rm = mad(mom, mean, (f32(1) - mom) * rm, self.fused)
      rv = mad(mom, unbf, (f32(1) - mom) * rv, self.fused)
      nbt0 += 1
    else:
      mean, var = rm, rv
    invstd = (1.0 / np.sqrt((var + eps).astype(f64))).astype(f32)
    sc = gamma * invstd
    sh = mad(-mean, sc, beta, self.fused)
    return torch.from_numpy(np.stack([sc, sh, mean, invstd, unbf])), torch.from_numpy(rm), torch.from_numpy(rv), nbt0

  def bwd_finalize(self, sums, gamma, mean, invstd, count):
    s, sy = sums[0].numpy().astype(f64), sums[1].numpy().astype(f64)
    mu, inv, g = mean.numpy().astype(f64), invstd.numpy().astype(f64), gamma.numpy().astype(f64)
    sgx = (sy - mu * s) * inv                         # (mu * s is exact in float64: fused or not is the same)
    c1 = g * inv
    c2 = -c1 * sgx * inv / count
    if self.fused:
      c3 = np.array([float(Fraction(float(a)) - Fraction(float(b)) * Fraction(float(c))) for a, b, c in zip(-c1 * s / count, c2, mu)])
    else:
      c3 = -c1 * s / count - c2 * mu
    t = lambda a: torch.from_numpy(a.astype(f32))
    return torch.stack([t(c1), t(c2), t(c3)]), t(sgx), t(s)


EMUS = [pytest.param(True, id="fused"), pytest.param(False, id="unfused")]


@pytest.mark.parametrize("fused", EMUS)
@pytest.mark.parametrize("shape", cases.SHAPES + cases.FIRST_GEN_SHAPES, ids=str)
def test_correct_apply_kernels_stay_inside_the_bounds(shape, fused):
  """(a) and (c) on every shape of the GPU file, the walker in `act` mode (the instrumented library's case) included."""
  be = Emu(fused)
  cases.check_apply(be, shape)
  cases.check_bwd_apply(be, shape)
  if cases.check_c(shape[4]):
    cases.check_bwd_apply(be, shape, modes=("act",), gen2=True)


@pytest.mark.parametrize("fused", EMUS)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_correct_reduction_stays_inside_the_bound(shape, fused):
  """(b), with the precondition on the kept fraction of the masks."""
  cases.check_reduce(Emu(fused), shape)


@pytest.mark.parametrize("fused", EMUS)
def test_correct_finalisers_stay_inside_the_bounds(fused):
  """(d): every count, the eval-mode coefficients (and bn_apply with them), the backward finaliser."""
  be = Emu(fused)
  for count, ucount in cases.FIN_COUNTS:
    assert cases.check_finalize(be, count, ucount) <= 3.0
  coef = cases.check_finalize_eval(be)
  shape = (2, 5, 7, 1, cases.FIN_C)
  cases.check_apply_with(be, shape, cases.inputs(*shape)["y"], coef, None, None, None, 1, "eval")
  cases.check_bwd_finalize(be)


@pytest.mark.parametrize("shape", [(6, 13, 13, 1, 128), (3, 3, 5, 2, 64)], ids=str)
def test_boundary_data_discriminates_and_each_contraction_is_self_consistent(shape):
  """(f): the precondition (the unfused predicate and the exact sign differ on at least 10 % of the elements), the fused
  and the unfused kernels really disagree with each other on this data, and each on its own keeps the property the GPU
  test asserts: the mask recomputed from y equals the mask read from the stored activation."""
  y, coef, differ = cases.boundary_inputs(*shape)
  assert differ >= 0.10
  i = cases.inputs(*shape)
  acts = {}
  for fused in (True, False):
    be = Emu(fused)
    acts[fused] = be.apply(y, coef, None, None, None, 1, shape)
    a = be.reduce(i["dout"], acts[fused], y, None, None, shape)[0]
    m = be.reduce(i["dout"], None, y, None, coef, shape)[0]
    assert torch.equal(a, m)
    da = be.bwd_apply(i["dout"], acts[fused], y, i["b1"], None, None, None, shape, False)[0]
    dm = be.bwd_apply(i["dout"], None, y, i["b1"], None, None, coef, shape, False)[0]
    assert torch.equal(da, dm)
  assert float(((acts[True] > 0) != (acts[False] > 0)).float().mean()) >= 0.10


# --------------------------------------------------------------------------------------
# seeded defects
# --------------------------------------------------------------------------------------
OLD_SHAPE = (6, 13, 13, 1, 128)


def _old_criterion_rejects(defect):
  """test_bn_forward_backward_kernels restated on the emulation: its shape, its kind of data (y = 1.5 n + 0.3, batch
  statistics, gamma = 1 + 0.2 n, beta = 0.1 n), its paths (apply with a residual, apply with a second BatchNorm, the
  backward in `act` mode, then mask-from-y against mask-from-act) and its criteria.  True if any of them fails."""
  N, H, W, P, C = OLD_SHAPE
  rng = np.random.default_rng(7)
  r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(f32))
  y, y2, res, dout = cases.bf16(r(N, H, W, C) * 1.5 + 0.3), cases.bf16(r(N, H, W, C)), cases.bf16(r(N, H, W, C)), cases.bf16(r(N, H, W, C))
  gamma, beta = 1 + 0.2 * r(C), 0.1 * r(C)
  cnt = N * H * W

  def coef_of(t, g, b):
    m, v = t.double().mean((0, 1, 2)), t.double().var((0, 1, 2), unbiased=False)
    inv = (v + 1e-5).rsqrt()
    return torch.stack([g.double() * inv, b.double() - m * g.double() * inv, m, inv, v]).float()
  coef, coef2 = coef_of(y, gamma, beta), coef_of(y2, beta + 1.0, gamma * 0.1)
  be, good = Emu(True, defect), Emu(True)
  bad = False
  c, c2 = coef.double(), coef2.double()
  ref = (y.double() * c[0] + c[1] + res.double()).clamp_min(0)
  bad |= float((be.apply(y, coef, res, None, None, 1, OLD_SHAPE).double() - ref).abs().max()) > 2e-2
  ref2 = (y.double() * c[0] + c[1] + y2.double() * c2[0] + c2[1]).clamp_min(0)
  bad |= float((be.apply(y, coef, None, y2, coef2, 1, OLD_SHAPE).double() - ref2).abs().max()) > 2e-2
  # backward of relu(bn(y) + res) in float64
  act = cases.bf16(ref.float())
  g = torch.where(ref > 0, dout.double(), torch.zeros((), dtype=torch.float64))
  xhat = (y.double() - c[2]) * c[3]
  db, dg = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
  dy = gamma.double() * c[3] * (g - db / cnt - xhat * dg / cnt)
  s, _ = be.reduce(dout, act, y, None, None, OLD_SHAPE)
  bcoef, dgam, dbet = good.bwd_finalize(s.float(), gamma, coef[2], coef[3], cnt)
  bad |= not torch.allclose(dgam.double(), dg, rtol=2e-3, atol=2e-3 * float(dg.abs().max()))
  bad |= not torch.allclose(dbet.double(), db, rtol=2e-3, atol=2e-3 * float(db.abs().max()))
  got = be.bwd_apply(dout, act, y, bcoef, None, None, None, OLD_SHAPE, False)[0]
  bad |= float((got.double() - dy).abs().max()) > 1e-2 * float(dy.abs().max())
  # the mask recomputed from y against the mask read from act = relu(bn(y))
  a_plain = be.apply(y, coef, None, None, None, 1, OLD_SHAPE)
  s_a, s_m = be.reduce(dout, a_plain, y, None, None, OLD_SHAPE)[0], be.reduce(dout, None, y, None, coef, OLD_SHAPE)[0]
  bad |= not torch.allclose(s_a, s_m, rtol=1e-5, atol=1e-4)
  bc_a = good.bwd_finalize(s_a.float(), gamma, coef[2], coef[3], cnt)[0]
  try:
    bad |= not torch.equal(be.bwd_apply(dout, a_plain, y, bc_a, None, None, None, OLD_SHAPE, False)[0],
                           be.bwd_apply(dout, None, y, bc_a, None, None, coef, OLD_SHAPE, False)[0])
  except AssertionError:      # (the emulation's own border check: the old test looks at the border too)
    bad = True
  return bool(bad)


def test_old_criterion_accepts_the_correct_emulation():
  assert _old_criterion_rejects(None) is False


def _rejected(check, *args, **kw):
  with pytest.raises(AssertionError):
    check(*args, **kw)


def test_defect_tail_pixel_dropped_is_rejected():
  """`if (q < q1)` after the pair loop lost: the reduction misses pixels and the walker apply leaves them unwritten --
  rejected by (b) and (c) at (5,49,49,1,64) (last chunk of 37) and at (11,7,7,1,512) (last chunk of 3).
  Old criterion at the old shape: also rejected (its last chunk of 22 pixels over 16 lanes has a tail: computed below)."""
  be = Emu(True, "tail_dropped")
  for shape in ((5, 49, 49, 1, 64), (11, 7, 7, 1, 512)):
    _rejected(cases.check_reduce, be, shape)
    _rejected(cases.check_bwd_apply, be, shape, modes=("none",))
  assert _old_criterion_rejects("tail_dropped") is OLD["tail_dropped"]


def test_defect_border_skip_of_half_the_width_is_rejected():
  """px_advance skips P*C instead of 2*P*C at a row end: rejected by (b) and (c) wherever a walk crosses a row.
  Old criterion: also rejected (W = 13 < PL = 16: every step crosses a row and the sums are far off)."""
  be = Emu(True, "border_skip")
  for shape in ((6, 13, 13, 1, 128), (3, 3, 5, 2, 64), (2, 3, 5, 1, 2048)):
    _rejected(cases.check_reduce, be, shape)
    _rejected(cases.check_bwd_apply, be, shape, modes=("mask_coef",))
  assert _old_criterion_rejects("border_skip") is OLD["border_skip"]


def test_defect_ge_for_gt_in_the_mask_is_rejected():
  """`>=` for `>`: in both predicates, and in the one recomputed from y alone.  Rejected by (b) and (c): the inputs hold
  zeros of either sign in act and exact zeros of scale*y + shift.
  Old criterion: rejects the defect when it is in the `act` predicate (relu output is never negative, so every element
  passes), but does NOT reject it in the predicate recomputed from y: its random data has no element with
  scale*y + shift == 0, so both masks still agree."""
  for defect in ("mask_ge", "mask_ge_coef"):
    be = Emu(True, defect)
    for shape in ((6, 13, 13, 1, 128), (1, 1, 1, 1, 64)):
      _rejected(cases.check_reduce, be, shape)
      _rejected(cases.check_bwd_apply, be, shape, modes=("mask_coef",))
    assert _old_criterion_rejects(defect) is OLD[defect]


def test_defect_shift2_omitted_is_rejected():
  """The shared-downsample branch without its shift: rejected by (a).  Old criterion: also rejected (shift2 there is of
  the order of 0.1, five times its 2e-2)."""
  _rejected(cases.check_apply, Emu(True, "shift2_omitted"), (1, 1, 1, 1, 64))
  assert _old_criterion_rejects("shift2_omitted") is OLD["shift2_omitted"]


def test_defect_coefficient_of_channel_c_plus_8_is_rejected():
  """Channel c reads the coefficient of channel c + 8: rejected by (a) and (c).  Old criterion: also rejected."""
  be = Emu(True, "coef_plus8")
  _rejected(cases.check_apply, be, (1, 1, 1, 1, 64))
  _rejected(cases.check_bwd_apply, be, (2, 3, 5, 1, 2048), modes=("none",))
  assert _old_criterion_rejects("coef_plus8") is OLD["coef_plus8"]


# what the docstrings above state about the old criterion; _old_criterion_rejects must agree
OLD = {"tail_dropped": True, "border_skip": True, "mask_ge": True, "mask_ge_coef": False, "shift2_omitted": True,
       "coef_plus8": True}
DEFECTS = tuple(OLD)
