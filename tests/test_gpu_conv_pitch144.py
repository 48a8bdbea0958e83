"""The weights-direct conv kernels' two LDS patch forms (csrc/conv_igemm_bd.hip, conv_igemm_pw.hip, template PAD): rows at
a 144-byte pitch read with immediate offsets against the XOR-swizzled 128-byte rows.  Same MFMA sequence, same operands:
every output buffer, statistic cell and fused-reduction cell must carry the same bits (iic_debug_bd_pitch144 0 / 1).

Shapes: the smallest that reach every address class --
  3 x 13 x 13, 128 -> 128: two 64-channel chunks (one patch reload), dense row numbering with a 256-row tile that
                           straddles images, a ragged last tile (507 rows);
  2 x  7 x  7, 256 -> 256: four chunks, one tile larger than all the rows there are (98), the patch clamped at the
                           input's last pixel;
  5 x 25 x 25, 128 -> 128: 13 tiles; on the persistent kernel with one workgroup per XCD a workgroup walks two tiles
                           (the next tile's patch fetched under the epilogue, both key-less buffers' turn-around).
Kernels: "bd4" = conv_igemm_bd_kernel with 256-row tiles (iic_debug_bd_ms 4), "bd2" = the 128-row tiles its heuristic
picks for launches this small, "pw" = conv_igemm_pw_kernel (iic_debug_enable_pw 2: however few tiles;
iic_debug_pw_gx_cap 1).  iic_debug_bd_pitch144_used says which kernel reads a padded patch under the switches in force."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conftest import hook

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]

P = 1
SHAPES = {"13": (3, 13, 128, 128), "7": (2, 7, 256, 256), "25": (5, 25, 128, 128)}
KERNEL_ID = {"bd4": 1, "bd2": 1, "pw": 2}


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


def _bf16_with_zeros(rng, shape):
  """Seeded normal values rounded to bf16 (negative ones included), every eighth or so an exact zero."""
  x = rng.standard_normal(shape).astype(np.float32)
  x[rng.random(shape) < 0.125] = 0.0
  return torch.from_numpy(x).to(torch.bfloat16).float()


_CASES = {}


def _case(key):
  """Inputs of one shape, built once and shared (never modified) by the tests that use it."""
  if key not in _CASES:
    from iic_amd import geom, ops
    N, H, cin, cout = SHAPES[key]
    rng = np.random.default_rng(144 + H)
    x = _bf16_with_zeros(rng, (N, cin, H, H))
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32))
    dy = _bf16_with_zeros(rng, (N, cout, H, H))
    spec = geom.ConvSpec(cin, cout, 3, 1, 1)
    c = dict(N=N, H=H, cin=cin, cout=cout, x=x, w=w,
             gf=geom.fwd_geom(spec, N, H, H, P, P), gb=geom.bwd_data_geoms(spec, N, H, H, P, P),
             xp=ops.pt_from_nchw(x.to(dev()), P), dyp=ops.pt_from_nchw(dy.to(dev()), P),
             res=ops.pt_from_nchw(_bf16_with_zeros(rng, (N, cin, H, H)).to(dev()), P),
             act=ops.pt_from_nchw(_bf16_with_zeros(rng, (N, cin, H, H)).to(dev()), P),
             prev=ops.pt_from_nchw(_bf16_with_zeros(rng, (N, cin, H, H)).to(dev()), P),
             coef=torch.stack([torch.from_numpy(rng.random(cin).astype(np.float32)) + 0.5,
                               torch.from_numpy(rng.standard_normal(cin).astype(np.float32)) * 0.3,
                               torch.zeros(cin), torch.ones(cin), torch.zeros(cin)]).to(dev()),
             pw=ops.PreppedWeights(w.to(dev())))
    assert len(c["gb"]) == 1
    _CASES[key] = c
  return _CASES[key]


def _lib():
  from iic_amd import _lib as L
  h = ctypes.CDLL(L.LIB_PATH)
  h.iic_debug_bd_pitch144_used.restype = ctypes.c_int
  h.iic_debug_get_bd_pitch144.restype = ctypes.c_int
  return h


class _Forms(object):
  """Run `fn` under both patch forms on one kernel; restores every switch it touched."""

  def __init__(self, kernel):
    self.kernel = kernel
    self.default = _lib().iic_debug_get_bd_pitch144()

  def __enter__(self):
    if self.kernel == "bd4":
      hook("iic_debug_bd_ms", 4)
    elif self.kernel == "bd2":
      hook("iic_debug_enable_pw", 0)
    else:
      hook("iic_debug_enable_pw", 2)
      hook("iic_debug_pw_gx_cap", 1)
    return self

  def __exit__(self, *exc):
    hook("iic_debug_bd_pitch144", self.default)
    hook("iic_debug_bd_ms", 0)
    hook("iic_debug_enable_pw", 1)
    hook("iic_debug_pw_gx_cap", 0)
    return False

  def both(self, g, fn):
    out = {}
    for form in (0, 1):
      hook("iic_debug_bd_pitch144", form)
      g._frag_ok = g._red_ok = None
      used = _lib().iic_debug_bd_pitch144_used(ctypes.byref(g))
      assert used == (KERNEL_ID[self.kernel] if form else 0), (self.kernel, form, used)
      out[form] = fn()
      torch.cuda.synchronize()
    return out[0], out[1]


def _assert_same_bits(swz, pad):
  assert len(swz) == len(pad)
  for i, (a, b) in enumerate(zip(swz, pad)):
    assert torch.equal(a, b), "output %d differs between the patch forms" % i


def _assert_border_zero(t):
  assert float(t[:, :P].abs().max()) == 0.0 and float(t[:, -P:].abs().max()) == 0.0
  assert float(t[:, :, :P].abs().max()) == 0.0 and float(t[:, :, -P:].abs().max()) == 0.0


@pytest.mark.parametrize("key,kernel", [("13", "bd4"), ("13", "bd2"), ("7", "bd4"), ("7", "pw"), ("25", "pw"), ("25", "bd4")])
def test_forward_patch_forms_are_bit_identical(key, kernel):
  """Forward with the fused BatchNorm statistics: the whole PT output (its zero border included, which must stay zero)
  and the exact statistic cells, bit for bit between the two forms; the padded form also against F.conv2d."""
  from iic_amd import ops
  c = _case(key)

  def run():
    y = torch.zeros(c["N"], c["H"] + 2 * P, c["H"] + 2 * P, c["cout"], dtype=torch.bfloat16, device=dev())
    st = ops.new_stats(c["cout"], dev())
    ops.conv_igemm(c["gf"], c["xp"], c["pw"][0], y, stats=st)
    return y, st

  with _Forms(kernel) as f:
    swz, pad = f.both(c["gf"], run)
  _assert_same_bits(swz, pad)
  _assert_border_zero(pad[0])
  ref = F.conv2d(c["x"], c["w"].to(torch.bfloat16).float(), stride=1, padding=1)
  got = ops.pt_to_nchw(pad[0], P).cpu()
  assert (got - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()


@pytest.mark.parametrize("key,kernel", [("13", "bd4"), ("25", "pw")])
@pytest.mark.parametrize("epilogue", ["res_premask", "accumulate", "red"])
def test_backward_data_patch_forms_are_bit_identical(key, kernel, epilogue):
  """Backward-data with each fused epilogue -- residual gradient + pre-masked ReLU, accumulate onto previous contents,
  the BatchNorm-backward reduction -- dx as a whole PT buffer and, for the reduction, its sum cells: bit for bit."""
  from iic_amd import ops
  c = _case(key)
  g = c["gb"][0]

  def run():
    dx = torch.zeros(c["N"], c["H"] + 2 * P, c["H"] + 2 * P, c["cin"], dtype=torch.bfloat16, device=dev())
    if epilogue == "res_premask":
      ops.conv_igemm(g, c["dyp"], c["pw"][1], dx, res_grad=c["res"], res_act=c["act"], premask=True)
      return (dx,)
    if epilogue == "accumulate":
      dx.copy_(c["prev"])
      ops.conv_igemm(g, c["dyp"], c["pw"][1], dx, accumulate=True)
      return (dx,)
    assert ops.red_supported(g, c["pw"][1])
    s1 = ops.new_stats(c["cin"], dev())
    ops.conv_igemm(g, c["dyp"], c["pw"][1], dx, red=(c["xp"], c["coef"], s1, None, None))
    return dx, s1

  with _Forms(kernel) as f:
    swz, pad = f.both(g, run)
  _assert_same_bits(swz, pad)
  _assert_border_zero(pad[0])
  assert float(pad[0].float().abs().max()) > 0.0
  if epilogue == "red":
    assert bool((pad[1] != 0).any())
