"""The persistent 64 -> 64 conv kernel's two tile-loop forms (csrc/conv_igemm_p64.hip, template FORM, switch
iic_debug_p64_form): 1 = closed-form patch addresses, incremental row tables, the next patch's DMA and the next table
issued inside the K loop, the patch rows read one tile ahead; 0 = the first form.  Same MFMA sequence, same operands:
every output buffer (border included), statistic cell and fused-reduction cell must carry the same bits.

Every case is 64 -> 64, 3 x 3, pad 1, stride 1; the smallest shapes at which each mechanism can go wrong --
  1 x  7 x  7 (M = 49):  one partial tile; the tables of tiles t0 + 1, t0 + 2 lie wholly past the end; rows >= M are
                         never stored and do not count in the statistics;
  3 x 13 x 13 (M = 507): two tiles, both straddle image boundaries (the walker's 2-row pad skip), the last one partial;
  2 x 49 x 49, grid 2:   9-10 tiles per workgroup: the 4-slot table ring wraps twice, both patch buffers are reused, the
                         last workgroup's DMA is clamped at the tensor's last pixel;
  5 x 25 x 25, grid 3:   uneven tile ranges per workgroup (4, 4, 5), a row length other than the layer's own.
One float64 assertion on the 13 x 13 case anchors the identity (two equally wrong kernels would pass it otherwise).  Its
bound is in the units of tests/parity.py: the 576 products are exact in fp32, each of the 576 fp32 accumulations costs at
most U32 of the magnitude sum A = sum |x| |w| (parity.conv_acc_bound), and the round-to-nearest-even store must then land in
parity.bf16_bracket(ref, 576 U32 A), which lies inside the earlier 576 U32 A + U16 |ref|."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import hook
from tests.parity import U16, assert_in_bracket, assert_within, bf16_bracket, conv_acc_bound

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]

P = 1
C = 64
CASES = {"7": (1, 7, 0), "13": (3, 13, 0), "49": (2, 49, 2), "25": (5, 25, 3)}     # N, H, forced grid
MODES = ["fwd_stats", "bwd_plain", "bwd_res_premask", "bwd_accumulate"]


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


def _bf16_unit(rng, shape):
  """Seeded values in [-1, 1] rounded to bf16: about half of them negative, so a ReLU mask taken from them is mixed."""
  return torch.from_numpy(rng.uniform(-1.0, 1.0, shape).astype(np.float32)).to(torch.bfloat16).float()


_BUILT = {}


def _case(key):
  """Inputs of one shape, built once and shared (never modified) by the tests that use it."""
  if key not in _BUILT:
    from iic_amd import geom, ops
    N, H, grid = CASES[key]
    rng = np.random.default_rng(6400 + H)
    x = _bf16_unit(rng, (N, C, H, H))
    w = torch.from_numpy((rng.uniform(-1.0, 1.0, (C, C, 3, 3)) / 24.0).astype(np.float32))
    spec = geom.ConvSpec(C, C, 3, 1, 1)
    pt = lambda: ops.pt_from_nchw(_bf16_unit(rng, (N, C, H, H)).to(dev()), P)
    c = dict(N=N, H=H, grid=grid, x=x, w=w, gf=geom.fwd_geom(spec, N, H, H, P, P),
             gb=geom.bwd_data_geoms(spec, N, H, H, P, P), xp=ops.pt_from_nchw(x.to(dev()), P), dyp=pt(), res=pt(),
             act=pt(), prev=pt(),
             coef=torch.stack([torch.from_numpy(rng.random(C).astype(np.float32)) + 0.5,
                               torch.from_numpy(rng.standard_normal(C).astype(np.float32)) * 0.3,
                               torch.zeros(C), torch.ones(C), torch.zeros(C)]).to(dev()),
             pw=ops.PreppedWeights(w.to(dev())))
    assert len(c["gb"]) == 1
    _BUILT[key] = c
  return _BUILT[key]


def _plan(g):
  from iic_amd import _lib
  out = (ctypes.c_int * 12)()
  ctypes.CDLL(_lib.LIB_PATH).iic_debug_conv_plan(ctypes.byref(g), out)
  return list(out)


def _both_forms(c, g, fn, red=False):
  """fn() under form 0 and form 1 on the persistent kernel with the case's grid; restores every switch it touched."""
  out = {}
  try:
    hook("iic_debug_p64_grid", c["grid"])
    if red:
      hook("iic_debug_p64_red", 1)
    g._frag_ok = g._red_ok = None
    plan = _plan(g)
    tiles = (c["N"] * c["H"] * c["H"] + 255) // 256
    assert plan[0] == 1 and plan[7] == tiles and plan[8] == (c["grid"] or tiles), plan
    for form in (0, 1):
      hook("iic_debug_p64_form", form)
      out[form] = fn()
      torch.cuda.synchronize()
  finally:
    hook("iic_debug_p64_form", 1)
    hook("iic_debug_p64_grid", 0)
    hook("iic_debug_p64_red", 0)
    g._frag_ok = g._red_ok = None
  return out[0], out[1]


def _assert_same_bits(first, new):
  assert len(first) == len(new)
  for i, (a, b) in enumerate(zip(first, new)):
    assert torch.equal(a, b), "output %d differs between the tile-loop forms" % i


def _assert_border_zero(t):
  assert float(t[:, :P].abs().max()) == 0.0 and float(t[:, -P:].abs().max()) == 0.0
  assert float(t[:, :, :P].abs().max()) == 0.0 and float(t[:, :, -P:].abs().max()) == 0.0


def _new_pt(c):
  return torch.zeros(c["N"], c["H"] + 2 * P, c["H"] + 2 * P, C, dtype=torch.bfloat16, device=dev())


def _run(c, mode):
  from iic_amd import ops
  g = c["gb"][0]
  out = _new_pt(c)
  if mode == "fwd_stats":
    st = ops.new_stats(C, dev())
    ops.conv_igemm(c["gf"], c["xp"], c["pw"][0], out, stats=st)
    return out, st
  if mode == "bwd_plain":
    ops.conv_igemm(g, c["dyp"], c["pw"][1], out)
    return (out,)
  if mode == "bwd_res_premask":
    ops.conv_igemm(g, c["dyp"], c["pw"][1], out, res_grad=c["res"], res_act=c["act"], premask=True)
    return (out,)
  if mode == "bwd_accumulate":
    out.copy_(c["prev"])
    ops.conv_igemm(g, c["dyp"], c["pw"][1], out, accumulate=True)
    return (out,)
  assert mode == "bwd_red" and ops.red_supported(g, c["pw"][1])
  s1 = ops.new_stats(C, dev())
  ops.conv_igemm(g, c["dyp"], c["pw"][1], out, red=(c["xp"], c["coef"], s1, None, None))
  return out, s1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(CASES))
def test_tile_loop_forms_are_bit_identical(key, mode):
  """Forward with the fused BatchNorm statistics and backward-data plain / residual + pre-masked ReLU / accumulate: the
  whole PT buffer (its border must stay zero) and the exact statistic cells, bit for bit between the two forms."""
  c = _case(key)
  first, new = _both_forms(c, c["gf"] if mode == "fwd_stats" else c["gb"][0], lambda: _run(c, mode))
  _assert_same_bits(first, new)
  _assert_border_zero(new[0])
  assert float(new[0].float().abs().max()) > 0.0
  if mode == "fwd_stats":
    assert bool((new[1] != 0).any())
  if mode == "bwd_res_premask":
    frac = float((new[0][:, P:-P, P:-P] == 0).float().mean())
    assert 0.2 < frac < 0.8, frac      # the mask is mixed


@pytest.mark.parametrize("key", ["13", "49"])
def test_tile_loop_forms_are_bit_identical_with_the_fused_reduction(key):
  """Backward-data with the BatchNorm-backward reduction in the epilogue (iic_debug_p64_red 1): dx and the sum cells."""
  c = _case(key)
  first, new = _both_forms(c, c["gb"][0], lambda: _run(c, "bwd_red"), red=True)
  _assert_same_bits(first, new)
  _assert_border_zero(new[0])
  assert bool((new[1] != 0).any())


def test_new_form_matches_float64_convolution():
  """Form 1, forward, 3 x 13 x 13, against F.conv2d in float64 on the bf16-rounded operands: the fp32 accumulator lies
  within conv_acc_bound(576, A) = 576 U32 A of it, so the stored value lies in bf16_bracket(ref, 576 U32 A)
  (tests/parity.py) -- inside the earlier 576 U32 A + U16 |ref|, which is asserted as well."""
  from iic_amd import ops
  c = _case("13")
  _, new = _both_forms(c, c["gf"], lambda: _run(c, "fwd_stats"))
  xd, wd = c["x"].double(), c["w"].to(torch.bfloat16).double()
  ref = F.conv2d(xd, wd, stride=1, padding=1)
  A = F.conv2d(xd.abs(), wd.abs(), stride=1, padding=1)
  b = conv_acc_bound(576, A)
  lo, hi = bf16_bracket(ref, b)
  got = ops.pt_to_nchw(new[0], P).float()
  assert_in_bracket(got, lo, hi, "p64 form 1 forward", "conv64 forward p64-forms mixed", ref=ref, b=b)
  assert_within(got, ref, b + U16 * ref.abs(), "p64 form 1 forward")
