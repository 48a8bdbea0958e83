"""The product bf16 BatchNorm kernels of csrc/bn.hip and the exact statistic cells of csrc/common.h against float64.

Conventions of tests/test_gpu_kernels_f64.py: float64 references on the CPU, U32 = 2^-24 per fp32 operation, U16 = 2^-8
per bf16 store times |ref|, outputs pre-filled with a sentinel and the border asserted untouched, C entry points called
directly.  Inputs, references and bounds live in tests/bn_bf16_cases.py; tests/test_bn_bf16_cpu.py proves there, on a
numpy emulation of the kernels, that the bounds admit the correct arithmetic and reject seeded one-term defects.

Shapes (N, H, W, P, C), one hazard each:
  (6,13,13,1,128)   the shape of test_bn_forward_backward_kernels
  (1,1,1,1,64)      one pixel, 31 of the 32 pixel lanes idle
  (3,3,5,2,64)      PL = 32 exceeds the 15 pixels of an image: one px_advance crosses two image borders, P = 2
  (2,20,36,2,64)    W*C/8 = 288 > 256: a second blockIdx.y in bn_apply and the first-generation backward apply
  (5,49,49,1,64)    12005 pixels in chunks of 64, a ragged last chunk of 37: pair loop plus tail
  (11,7,7,1,512)    PL = 4, chunks of 8, a last chunk of 3 pixels (fewer than PL)
  (3,5,3,1,1024), (2,3,5,1,2048)   PL = 2 and PL = 1
  (2,5,7,1,C), C = 8, 24, 192      check_c fails: first-generation kernels, no reduction
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import bn_bf16_cases as cases
from tests.conftest import hook
from tests.parity import SENTINEL, WORST, assert_border, call, dev, interior, ok, pt_of

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
IIC_ERR_UNSUPPORTED = -3
INVSTD_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
  """After the module: the worst |err| / bound per family (LAB.md records them); IIC_PARITY_REPORT names a JSON file."""
  yield
  rec = dict(worst_err_over_bound=dict(WORST), invstd_rel_err_in_u32=dict(INVSTD_WORST))
  print("\nparity report: " + json.dumps(rec, sort_keys=True))
  if os.environ.get("IIC_PARITY_REPORT"):
    with open(os.environ["IIC_PARITY_REPORT"], "w") as f:
      json.dump(rec, f, indent=1, sort_keys=True)


def _pt(x, P):
  return None if x is None else pt_of(x, P, BF16)


def _sentinel(shape):
  N, H, W, P, C = shape
  return torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, dtype=BF16, device=dev())


def _coef5(c):
  """[2, C] or [3, C] or [5, C] coefficients on the GPU ([5, C] rows beyond the given ones zero)."""
  return None if c is None else c.to(dev()).contiguous()


class Gpu:
  """The C entry points as a backend of tests/bn_bf16_cases.py; asserts the untouched border itself."""

  def apply(self, y, coef, res, y2, coef2, relu, shape):
    N, H, W, P, C = shape
    out = _sentinel(shape)
    ok("iic_bn_apply", _pt(y, P), _coef5(coef), _pt(res, P), _pt(y2, P), _coef5(coef2), out, N, H, W, P, C, relu)
    assert_border(out, P, SENTINEL, "bn_apply")
    return interior(out, P).float()

  def reduce_cells(self, dout, act, y, y2, mcoef, shape):
    from iic_amd import ops
    N, H, W, P, C = shape
    s1, s2 = ops.new_stats(C, dev()), ops.new_stats(C, dev())
    ok("iic_bn_bwd_reduce", _pt(dout, P), _pt(act, P), _pt(y, P), _pt(y2, P), s1, s2 if y2 is not None else None,
       _coef5(mcoef), N, H, W, P, C)
    return s1, (s2 if y2 is not None else None)

  def reduce(self, dout, act, y, y2, mcoef, shape):
    from iic_amd import ops
    s1, s2 = self.reduce_cells(dout, act, y, y2, mcoef, shape)
    C = shape[4]
    return ops.stats_decode(s1, C).cpu(), (ops.stats_decode(s2, C).cpu() if s2 is not None else None)

  def bwd_apply_pt(self, dout, act, y, b1, y2, b2, mcoef, shape):
    N, H, W, P, C = shape
    dy, dy2 = _sentinel(shape), _sentinel(shape)
    ok("iic_bn_bwd_apply", _pt(dout, P), _pt(act, P), _pt(y, P), _coef5(b1), dy, _pt(y2, P), _coef5(b2),
       dy2 if y2 is not None else None, _coef5(mcoef), N, H, W, P, C)
    assert_border(dy, P, SENTINEL, "bn_bwd_apply dy")
    assert_border(dy2, P, SENTINEL, "bn_bwd_apply dy2")
    if y2 is None:
      assert bool((dy2.float() == SENTINEL).all()), "dy2 written without y2"
    return dy, dy2

  def bwd_apply(self, dout, act, y, b1, y2, b2, mcoef, shape, gen2):
    dy, dy2 = self.bwd_apply_pt(dout, act, y, b1, y2, b2, mcoef, shape)
    P = shape[3]
    return interior(dy, P).float(), (interior(dy2, P).float() if y2 is not None else None)

  def finalize(self, sums, gamma, beta, rm0, rv0, nbt0, count, ucount, training):
    from iic_amd import ops
    C = gamma.shape[0]
    st = None
    if training:
      st = ops.new_stats(C, dev())
      ops.stats_encode(st, C, sums)
    rm, rv = rm0.clone().to(dev()), rv0.clone().to(dev())
    nbt = torch.full((), nbt0, dtype=torch.long, device=dev())
    coef = torch.full((5, C), SENTINEL, device=dev())
    ok("iic_bn_finalize", st, gamma.to(dev()), beta.to(dev()), rm, rv, nbt, coef, C, count, ucount,
       ctypes.c_float(cases.BN_EPS), ctypes.c_float(cases.MOMENTUM), training)
    if training:
      assert int(st.abs().max()) == 0, "the accumulator is not zero after iic_bn_finalize"
    return coef.cpu(), rm.cpu(), rv.cpu(), int(nbt)

  def bwd_finalize(self, sums, gamma, mean, invstd, count):
    from iic_amd import ops
    C = gamma.shape[0]
    st = ops.new_stats(C, dev())
    ops.stats_encode(st, C, sums)
    coef = torch.stack([torch.zeros(C), torch.zeros(C), mean, invstd, torch.zeros(C)]).to(dev())
    bcoef, dg, db = (torch.full(s, SENTINEL, device=dev()) for s in ((3, C), (C,), (C,)))
    ok("iic_bn_bwd_finalize", st, gamma.to(dev()), coef, bcoef, dg, db, C, count)
    assert int(st.abs().max()) == 0, "the accumulator is not zero after iic_bn_bwd_finalize"
    return bcoef.cpu(), dg.cpu(), db.cpu()


GPU = Gpu()


# --------------------------------------------------------------------------------------
# (a) - (c): the streaming kernels
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES + cases.FIRST_GEN_SHAPES, ids=str)
def test_bn_apply_vs_float64(shape):
  """iic_bn_apply, relu 0/1 x residual x shared-downsample branch, random fp32 coefficients: 6 * U32 * A + U16 * |ref|."""
  cases.check_apply(GPU, shape)


def test_bn_apply_with_eval_mode_coefficients_vs_float64():
  """iic_bn_finalize(training=0) against float64 on the running statistics, then iic_bn_apply with those coefficients."""
  coef = cases.check_finalize_eval(GPU)
  shape = (2, 5, 7, 1, cases.FIN_C)
  i = cases.inputs(*shape)
  for relu in (0, 1):
    cases.check_apply_with(GPU, shape, i["y"], coef, None, None, None, relu, "bn_apply with eval coefficients relu=%d" % relu)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_bn_bwd_reduce_vs_float64(shape):
  """iic_bn_bwd_reduce (the pixel walker bn_bwd_reduce2_kernel), three mask modes x with / without y2 + sums2:
  n_block * U32 * sum |terms| per channel; sums2[0] == sums[0] exactly."""
  cases.check_reduce(GPU, shape)


@pytest.mark.parametrize("shape", cases.FIRST_GEN_SHAPES, ids=str)
def test_bn_bwd_reduce_refuses_other_channel_counts(shape):
  """check_c fails: IIC_ERR_UNSUPPORTED and the accumulator untouched (all zero)."""
  from iic_amd import ops
  N, H, W, P, C = shape
  i = cases.inputs(*shape)
  st = ops.new_stats(C, dev())
  assert call("iic_bn_bwd_reduce", _pt(i["dout"], P), None, _pt(i["y"], P), None, st, None, None, N, H, W, P, C) == IIC_ERR_UNSUPPORTED
  assert int(st.abs().max()) == 0


@pytest.mark.parametrize("shape", cases.SHAPES + cases.FIRST_GEN_SHAPES, ids=str)
def test_bn_bwd_apply_vs_float64(shape):
  """iic_bn_bwd_apply as the product runs it -- `act` mode on the first-generation kernel, the other modes on the pixel
  walker bn_bwd_apply2_kernel (first generation where check_c fails) -- with and without dy2: 4 * U32 * A + U16 * |ref|."""
  cases.check_bwd_apply(GPU, shape)


@pytest.mark.hooks
@pytest.mark.parametrize("shape", cases.SHAPES, ids=str)
def test_bn_bwd_apply_second_generation_act_mode_vs_float64(shape):
  """iic_debug_bn_v2(2, 0): the pixel walker also where the mask is read from the activation tensor; the same bound."""
  hook("iic_debug_bn_v2", 2, 0)
  try:
    cases.check_bwd_apply(GPU, shape, modes=("act",), gen2=True)
  finally:
    hook("iic_debug_bn_v2", 1, 0)


# --------------------------------------------------------------------------------------
# (d) the finalisers
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,ucount", cases.FIN_COUNTS)
def test_bn_finalize_vs_float64(count, ucount):
  """iic_bn_finalize(training=1) per channel: ordinary data, a variance of 1/16 under a mean of 100, a constant channel
  (invstd = rsqrt(eps)), sums whose rounding makes ss/count - m^2 negative (clamped to 0); count = 1; an unbiased count
  of its own.  Bounds: tests/bn_bf16_cases.py check_finalize."""
  worst = cases.check_finalize(GPU, count, ucount)
  INVSTD_WORST["count=%d ucount=%d" % (count, ucount)] = worst


def test_bn_bwd_finalize_vs_float64():
  """iic_bn_bwd_finalize, sums with sy within a few ulps of mean*s and exactly on it (cancellation in sgx)."""
  cases.check_bwd_finalize(GPU)


# --------------------------------------------------------------------------------------
# (e) the accumulator's contract (csrc/common.h), through iic_bn_bwd_reduce in mask mode 0
# --------------------------------------------------------------------------------------
def _decode_then_finalize(st, C):
  """Decoded sums [2, C]; then iic_bn_bwd_finalize must leave every cell zero, the poison counter included."""
  from iic_amd import ops
  got = ops.stats_decode(st, C).cpu()
  coef = torch.ones((5, C), device=dev())
  bcoef, dg, db = torch.empty((3, C), device=dev()), torch.empty(C, device=dev()), torch.empty(C, device=dev())
  ok("iic_bn_bwd_finalize", st, torch.ones(C, device=dev()), coef, bcoef, dg, db, C, 1)
  assert int(st.abs().max()) == 0, "cells (or a poison counter) not zero after iic_bn_bwd_finalize"
  return got, db.cpu()


def test_stat_cells_documented_range_and_poison():
  """C = 2048: PL = 1 and, up to 512 pixels, every block takes a chunk of 2 pixels (restated from bn_v2_grid and asserted).
  The second pixel of every pair is 0, so block i's partial for a channel is exactly the bf16 value in pixel 2i; y = 1
  makes the second statistic the same.  Different channels carry different cases in one launch:
  {+2^60, -2^60, 2^-90} in three blocks decodes to exactly 2^-90; 2^-96 decodes exactly and 2^-97 to 0 (the documented
  loss below the lsb); 2^71 decodes exactly; inf, NaN and 2^100 (as g*y = 2^50 * 2^50) decode to NaN; every other
  channel -- the neighbours included -- is finite and exact."""
  N, H, W, P, C = 1, 4, 8, 1, 2048
  per, grid, PL = cases.v2_grid(N * H * W, C, 1)
  assert (per, grid, PL) == (2, 16, 1) and cases.v2_grid(512, C, 1)[0] == 2
  rng = np.random.default_rng(3)
  base = cases.bf16(torch.from_numpy(rng.integers(-64, 65, (H * W // 2, C)).astype(np.float32)) / 8)
  g = torch.zeros(H * W, C)
  g[0::2] = base                                          # pixel 2i: block i's whole partial
  y = torch.ones(H * W, C)
  special = {100: [(0, 2.0 ** 60), (5, -2.0 ** 60), (9, 2.0 ** -90)], 200: [(3, 2.0 ** -96)], 300: [(3, 2.0 ** -97)],
             400: [(7, 2.0 ** 71)], 500: [(2, float("inf"))], 600: [(11, float("nan"))], 700: [(4, 2.0 ** 50)]}
  for c, items in special.items():
    g[:, c] = 0
    for blk, v in items:
      g[2 * blk, c] = v
  y[2 * 4, 700] = 2.0 ** 50
  assert torch.equal(cases.bf16(g).nan_to_num(1.0), g.nan_to_num(1.0))
  st, _ = GPU.reduce_cells(g.view(N, H, W, C), None, y.view(N, H, W, C), None, None, (N, H, W, P, C))
  got, dbeta = _decode_then_finalize(st, C)
  want = torch.stack([g.double().sum(0), (g.double() * y.double()).sum(0)])
  want[:, 100], want[:, 300] = 2.0 ** -90, 0.0
  want[:, 500] = want[:, 600] = float("nan")
  want[0, 700], want[1, 700] = 2.0 ** 50, float("nan")
  assert int(torch.isnan(want).sum()) == 5
  assert bool((torch.isnan(got) == torch.isnan(want)).all()), "NaN where none is due, or none where one is"
  assert bool((got == want)[~torch.isnan(want)].all()), "a finite decoded sum is not exact"
  assert float(got[0, 200]) == 2.0 ** -96 and float(got[0, 400]) == 2.0 ** 71
  assert bool(torch.isnan(dbeta[[500, 600]]).all()) and float(dbeta[100]) == float(np.float32(2.0 ** -90))


@pytest.mark.parametrize("P", [0, 1])
@pytest.mark.parametrize("exp", [21, -3])
def test_stat_cells_carry_headroom(P, exp):
  """(1,16,32,P,2048): 256 blocks of 2 pixels add the same partial 2v, v = the largest bf16 mantissa at one exponent --
  with exp = 21 the partial's 24-bit mantissa is shifted by 23 bits, to the top of its bin -- and the decoded sum must be
  512 * v exactly, in both statistics."""
  N, H, W, C = 1, 16, 32, 2048
  assert cases.v2_grid(N * H * W, C, 1) == (2, 256, 1)
  v = 1.9921875 * 2.0 ** exp
  if exp == 21:        # fp32 exponent field of 2v is 127 + 22: lsb position 149 - 150 + 96 = 95 = 3 * 24 + 23
    assert (127 + exp + 1 - 150 + 96) % 24 == 23
  g = torch.full((N, H, W, C), v)
  assert torch.equal(cases.bf16(g), g)
  st, _ = GPU.reduce_cells(g, None, torch.ones_like(g), None, None, (N, H, W, P, C))
  got, _ = _decode_then_finalize(st, C)
  assert bool((got == 512 * v).all()), "carry lost: %r" % got[:, :4]


# --------------------------------------------------------------------------------------
# (f) every kernel takes the same side of the ReLU boundary
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_y2", [False, True])
@pytest.mark.parametrize("shape", [(6, 13, 13, 1, 128), (3, 3, 5, 2, 64)], ids=str)
def test_mask_from_y_agrees_with_the_stored_activation_on_boundary_data(shape, use_y2):
  """shift = -fl32(scale*y0) and a quarter of every channel's pixels at y0: there the fused multiply-add leaves the
  rounding residual of scale*y0 (either sign) and the unfused one leaves 0 -- asserted on the inputs: the two predicates
  differ on at least 10 % of all elements.  Whatever the kernels do, they must all do the same: act = iic_bn_apply(relu=1)
  stores relu(scale*y + shift), and the backward kernels that recompute the mask from y must leave the same integer
  cells (reduce) and the same bits (apply) as the ones that read act."""
  N, H, W, P, C = shape
  y, coef, differ = cases.boundary_inputs(*shape)
  assert differ >= 0.10, differ
  i = cases.inputs(*shape)
  act = GPU.apply(y, coef, None, None, None, 1, shape)
  y2 = i["y2"] if use_y2 else None
  ca, ca2 = GPU.reduce_cells(i["dout"], act, y, y2, None, shape)
  cm, cm2 = GPU.reduce_cells(i["dout"], None, y, y2, coef, shape)
  assert torch.equal(ca, cm), "bn_bwd_reduce: mask from y and mask from act leave different cells"
  if use_y2:
    assert torch.equal(ca2, cm2)
  b2 = i["b2"] if use_y2 else None
  da, da2 = GPU.bwd_apply_pt(i["dout"], act, y, i["b1"], y2, b2, None, shape)
  dm, dm2 = GPU.bwd_apply_pt(i["dout"], None, y, i["b1"], y2, b2, coef, shape)
  assert torch.equal(da, dm) and torch.equal(da2, dm2), "bn_bwd_apply: mask from y and mask from act differ"


@pytest.mark.parametrize("shape", [(6, 13, 13, 1, 128), (3, 3, 5, 2, 64)], ids=str)
def test_fused_bn_relu_maxpool_on_boundary_data(shape):
  """The same data through ops.bn_relu_maxpool2_fwd / _bwd against iic_bn_apply followed by the plain pool, bit for bit
  (tests/test_gpu_vgg.py does this on random data)."""
  from iic_amd import ops
  N, H, W, P, C = shape
  y, coef, differ = cases.boundary_inputs(*shape)
  assert differ >= 0.10
  Ho, Wo = H // 2, W // 2
  rng = np.random.default_rng(C)
  yp, cf = pt_of(y, P, BF16), coef.to(dev())
  dout = pt_of(cases.bf16(torch.from_numpy(rng.standard_normal((N, Ho, Wo, C)).astype(np.float32))), P, BF16)
  a = torch.zeros_like(yp)
  ops.bn_apply(yp, cf, a, N, H, W, P, C, relu=True)
  o_ref = torch.full((N, Ho + 2 * P, Wo + 2 * P, C), SENTINEL, dtype=BF16, device=dev())
  o_fus = o_ref.clone()
  ops.maxpool2_fwd(a, o_ref, N, H, W, P, P, C)
  ops.bn_relu_maxpool2_fwd(yp, cf, o_fus, N, H, W, P, P, C)
  d_ref, d_fus = _sentinel(shape), _sentinel(shape)
  ops.maxpool2_bwd(a, dout, d_ref, N, H, W, P, P, C)
  ops.bn_relu_maxpool2_bwd(yp, cf, dout, d_fus, N, H, W, P, P, C)
  torch.cuda.synchronize()
  assert torch.equal(o_ref, o_fus), "fused pool forward differs from the two-pass path"
  assert torch.equal(d_ref, d_fus), "fused pool backward differs from the two-pass path"
  assert_border(d_fus, P, SENTINEL, "fused pool backward")
