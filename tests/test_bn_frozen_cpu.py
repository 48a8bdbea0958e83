"""CPU proof of the bounds of tests/test_gpu_bn_frozen.py (kernel level): they must admit the correct one-pass backward of
a BatchNorm on running statistics and reject real defects.

bn_bwd_frozen_kernel / bn_bwd_finalize_frozen_kernel of csrc/bn.hip are emulated in numpy on top of the emulation of
tests/test_bn_bf16_cpu.py (its pixel walker, its chunked fp32 reduction, fused and unfused multiply-adds): the checks of
tests/bn_frozen_cases.py that the GPU file runs on the C entry points run here on the same inputs, then one defect at a
time is seeded and at least one bound must fail."""
import numpy as np
import pytest
import torch

from tests import bn_frozen_cases as fcases
from tests import test_bn_bf16_cpu as emu
from tests.parity import SENTINEL

f32, f64 = np.float32, np.float64
DEFECTS = ("mask_ignored", "invstd_for_scale", "coef_for_dy2", "mean_term_dropped", "not_rezeroed", "tail_skipped")


class FrozenEmu:
  """numpy emulation of the two kernels as a backend of tests/bn_frozen_cases.py.  defect: None or one of DEFECTS."""

  def __init__(self, fused, defect=None):
    self.fused, self.defect = fused, defect

  def frozen(self, dout, act, y, coef, y2, coef2, mcoef, shape):
    N, H, W, P, C = shape
    if self.defect == "mask_ignored":
      act = mcoef = None
    red = emu.Emu(self.fused, "tail_dropped" if self.defect == "tail_skipped" else None)
    s1, s2 = red.reduce(dout, act, y, y2, mcoef, shape)          # the same accumulation as bn_bwd_reduce2_kernel
    G, Y = emu._pad(emu._np(dout), P), emu._pad(emu._np(y), P)
    if act is not None or mcoef is not None:
      keep = red._keep(None if act is None else emu._pad(emu._np(act), P), Y, None if mcoef is None else emu._np(mcoef))
      G = np.where(keep, G, f32(0))
    at = emu.walk(shape, 1, drop_tail=self.defect == "tail_skipped").reshape(-1)   # the reduction's grid
    at = at[at >= 0]
    c1, c2 = emu._np(coef), emu._np(coef2)
    k1 = c1[3] if self.defect == "invstd_for_scale" else c1[0]
    outs = []
    for k in (k1,) + (((c1[0] if self.defect == "coef_for_dy2" else c2[0]),) if y2 is not None else ()):
      out = np.full_like(Y, SENTINEL)
      out[at] = emu._bf16((k * G[at]).astype(f32))               # one fp32 multiplication, one bf16 store
      out = out.reshape(N, H + 2 * P, W + 2 * P, C)
      border = np.ones(out.shape[1:3], dtype=bool)
      border[P:P + H, P:P + W] = False
      assert bool((out[:, border] == SENTINEL).all()), "the PT border was written"
      outs.append(torch.from_numpy(out[:, P:P + H, P:P + W].copy()))
    return outs[0], (outs[1] if y2 is not None else None), s1, s2

  def finalize_frozen(self, sums, coef):
    c = emu._np(coef)
    mu, inv = c[2].astype(f64), c[3].astype(f64)

    def run(cells):
      s, sy = cells[0], cells[1]
      mean_term = 0.0 if self.defect == "mean_term_dropped" else mu * s
      return ((sy - mean_term) * inv).astype(f32), s.astype(f32)
    cells = sums.numpy().astype(f64)
    dg, db = run(cells)
    if self.defect != "not_rezeroed":
      cells = np.zeros_like(cells)
    dg_b, db_b = run(cells)
    bcoef = np.stack([c[0], np.zeros_like(c[0]), np.zeros_like(c[0])])
    t = torch.from_numpy
    return t(bcoef), t(dg), t(db), t(dg_b), t(db_b)


EMUS = [pytest.param(True, id="fused"), pytest.param(False, id="unfused")]


@pytest.mark.parametrize("fused", EMUS)
@pytest.mark.parametrize("shape", fcases.SHAPES, ids=str)
def test_correct_one_pass_backward_stays_inside_the_bounds(shape, fused):
  fcases.check_frozen(FrozenEmu(fused), shape)


@pytest.mark.parametrize("fused", EMUS)
def test_correct_frozen_finaliser_stays_inside_the_bounds(fused):
  fcases.check_finalize_frozen(FrozenEmu(fused))


def test_shapes_reach_the_branches_they_were_chosen_for():
  """bn_v2_grid(reduce = 1) restated (bn_bf16_cases.v2_grid): pixels per block, blocks, pixel lanes."""
  g = lambda s: fcases.v2_grid(s[0] * s[1] * s[2], s[4], 1)
  assert g((1, 1, 1, 1, 64)) == (64, 1, 32)
  assert g((3, 3, 5, 2, 64)) == (64, 1, 32) and 45 - 32 == 13          # 13 lanes pair up, 19 take the tail alone
  assert g((2, 5, 7, 1, 128)) == (32, 3, 16)
  assert g((1, 7, 7, 1, 512)) == (8, 7, 4) and 49 - 6 * 8 == 1
  assert g((6, 13, 13, 1, 128)) == (32, 32, 16) and 1014 - 31 * 32 == 22
  assert all(not fcases.cases.check_c(C) for C in fcases.UNSUPPORTED_C)


def _rejected(check, *args, **kw):
  with pytest.raises(AssertionError):
    check(*args, **kw)


def test_defect_mask_ignored_is_rejected():
  """g = dout whatever the mask says: dy is not exact and the sums are off, in both masked modes, at every shape."""
  be = FrozenEmu(True, "mask_ignored")
  for shape in fcases.SHAPES:
    _rejected(fcases.check_frozen, be, shape, modes=("act",))
    _rejected(fcases.check_frozen, be, shape, modes=("mask_coef",))
  fcases.check_frozen(be, fcases.SHAPES[1], modes=("none",))       # (and only there)


def test_defect_invstd_for_scale_is_rejected():
  """dy = invstd * g (coef row 3) instead of scale * g (row 0)."""
  for shape in fcases.SHAPES:
    _rejected(fcases.check_frozen, FrozenEmu(True, "invstd_for_scale"), shape, modes=("none",))


def test_defect_first_coefficients_for_the_second_batchnorm_is_rejected():
  """dy2 = scale * g with the first BatchNorm's scale."""
  for shape in fcases.SHAPES:
    _rejected(fcases.check_frozen, FrozenEmu(True, "coef_for_dy2"), shape, modes=("none",))


def test_defect_running_mean_term_dropped_is_rejected():
  """dgamma = sum g*y * invstd, without running_mean * sum g."""
  _rejected(fcases.check_finalize_frozen, FrozenEmu(True, "mean_term_dropped"))


def test_defect_sums_not_rezeroed_is_rejected():
  """The finaliser leaves the accumulator as it found it: the next backward would add to stale sums."""
  _rejected(fcases.check_finalize_frozen, FrozenEmu(True, "not_rezeroed"))


def test_defect_pixel_skipped_at_the_pair_loops_tail_is_rejected():
  """`if (q < q1)` after the pair loop lost: at (3,3,5,2,64) 19 of the 45 pixels are neither written nor summed, at
  (1,1,1,1,64) the only one."""
  be = FrozenEmu(True, "tail_skipped")
  for shape in ((3, 3, 5, 2, 64), (1, 1, 1, 1, 64), (1, 7, 7, 1, 512)):
    _rejected(fcases.check_frozen, be, shape, modes=("none",))


def test_every_listed_defect_has_its_test():
  import sys
  names = [n for n in dir(sys.modules[__name__]) if n.startswith("test_defect_")]
  assert len(names) == len(DEFECTS)
