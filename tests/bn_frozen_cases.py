"""Inputs, float64 references and bounds for the backward of a BatchNorm on running statistics (csrc/bn.hip:
iic_bn_bwd_frozen, iic_bn_bwd_finalize_frozen), written once and used twice, as tests/bn_bf16_cases.py is:
tests/test_gpu_bn_frozen.py runs them against the C entry points, tests/test_bn_frozen_cpu.py against a numpy emulation
(the bounds admit the correct arithmetic and reject seeded defects).  A backend has

  frozen(dout, act, y, coef, y2, coef2, mcoef, shape) -> dy, dy2 | None, sums [2, C] float64, sums2 | None
  finalize_frozen(sums [2, C] fp32, coef [5, C]) -> bcoef [3, C], dgamma, dbeta, and dgamma, dbeta of a SECOND
                                                    finalise on the accumulator the first one left behind

on CPU tensors (interiors only, [N, H, W, C] float32 holding bf16 values).

No new number: dy is exact, the sums are held to the bound of bn_bf16_cases.check_reduce (the same accumulation: one
block's pixels in fp32, the blocks' partials exactly) and dgamma / dbeta to the bound of bn_bf16_cases.check_bwd_finalize
(a float64 formula on fp32 inputs, rounded once)."""
import torch

from tests import bn_bf16_cases as cases
from tests.bn_bf16_cases import EPS64, MASK_MODES, bf16, inputs, v2_grid
from tests.parity import U32, _masked_g, assert_within

# (N, H, W, P, C): the smallest shapes at which each branch of the pixel walker is reached
SHAPES = [(1, 1, 1, 1, 64),        # one pixel: 31 of 32 pixel lanes idle, the tail branch alone
          (3, 3, 5, 2, 64),        # 45 pixels over 32 lanes: 13 lanes take a pair, 19 the odd tail; P = 2
          (2, 5, 7, 1, 128),       # 70 pixels over 16 lanes, two blocks
          (1, 7, 7, 1, 512),       # 4 pixel lanes
          (6, 13, 13, 1, 128)]     # several blocks, a ragged last chunk
UNSUPPORTED_C = (8, 24, 192)       # check_c refuses them


def exact_dy(scale, g):
  """bf16(fp32(scale) * g): one fp32 multiplication, one round-to-nearest-even bf16 store."""
  return bf16(scale.float().view(1, 1, 1, -1) * g.float())


def assert_exact(got, want, what):
  bad = ~(got == want)             # (== : zeros of either sign compare equal)
  assert not bool(bad.any()), "%s: %d elements differ from bf16(scale * g), first at %s" % (
    what, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]))


def check_frozen(be, shape, modes=MASK_MODES):
  """Every mask mode, with and without the second BatchNorm: dy (dy2) exact, sums (sums2) within
  n_block * U32 * sum |terms| of the float64 sums, sums2[0] == sums[0]."""
  N, H, W, P, C = shape
  i = inputs(*shape)
  n_block = v2_grid(N * H * W, C, 1)[0]
  for mode in modes:
    if mode != "none":
      assert 0.2 < cases.keep_fraction(i, mode) < 0.8, (mode, cases.keep_fraction(i, mode))
    for use_y2 in (False, True):
      what = "bn_bwd_frozen %s mask=%s y2=%d" % (shape, mode, use_y2)
      dy, dy2, s1, s2 = be.frozen(i["dout"], i["act"] if mode == "act" else None, i["y"], i["coef"],
                                  i["y2"] if use_y2 else None, i["coef2"] if use_y2 else None,
                                  i["mcoef"] if mode == "mask_coef" else None, shape)
      g = _masked_g(i["dout"], i["act"], i["y"], i["mcoef"], mode)
      if mode != "none":
        assert bool((g == 0).any()) and bool((g != 0).any()), "the mask keeps everything or nothing"
      assert_exact(dy, exact_dy(i["coef"][0], g), what + " dy")
      if use_y2:
        assert_exact(dy2, exact_dy(i["coef2"][0], g), what + " dy2")
      else:
        assert dy2 is None and s2 is None
      gd = g.double()
      for st, yy in ((s1, i["y"]),) + (((s2, i["y2"]),) if use_y2 else ()):
        terms = torch.stack([gd, gd * yy.double()])
        assert_within(st, terms.sum((1, 2, 3)), n_block * U32 * terms.abs().sum((1, 2, 3)), what + " sums",
                      family="bn_bwd_frozen sums")
      if use_y2:
        assert torch.equal(s2[0], s1[0]), "sums2[0] != sums[0]"


def finalize_inputs():
  """The sums of bn_bf16_cases.bwd_finalize_inputs (sy within a few ulps of mean * s on the odd channels) under forward
  coefficients [5, C]: rows scale (gamma * invstd), shift, running mean, invstd, 0."""
  sums, mean, invstd, gamma = cases.bwd_finalize_inputs()
  scale = gamma * invstd
  coef = torch.stack([scale, 0.25 - mean * scale, mean, invstd, torch.zeros_like(mean)])
  return sums, coef


def check_finalize_frozen(be):
  """dgamma = (sy - mean * s) * invstd and dbeta = s within (U32 + 8 * EPS64) * |ref| of the float64 formula on the same
  fp32 inputs; bcoef = (coef row 0, 0, 0) bit for bit; a second finalise finds the accumulator re-zeroed."""
  sums, coef = finalize_inputs()
  bcoef, dgamma, dbeta, dgamma_b, dbeta_b = be.finalize_frozen(sums, coef)
  s, sy, mu, inv = sums[0].double(), sums[1].double(), coef[2].double(), coef[3].double()
  sgx = (sy - mu * s) * inv
  assert float((mu * s).abs().min()) > 0, "a channel without the running_mean * sum g term"
  for got, ref, what in ((dgamma, sgx, "dgamma"), (dbeta, s, "dbeta")):
    assert_within(got, ref, (U32 + 8 * EPS64) * ref.abs(), "bn_bwd_finalize_frozen " + what, family="bn_bwd_finalize_frozen")
  assert torch.equal(bcoef[0], coef[0]), "bcoef row 0 is not the forward scale"
  assert bool((bcoef[1:] == 0).all()), "bcoef rows 1, 2 are not zero"
  assert bool((dgamma_b == 0).all()) and bool((dbeta_b == 0).all()), "sums were not re-zeroed by the finaliser"
