"""Helpers shared by the float64 parity tests (tests/test_gpu_kernels_f64.py, tests/test_gpu_bn_bf16.py and the CPU proof of
the latter's bounds, tests/test_bn_bf16_cpu.py): direct calls of the C entry points, bit / bound comparisons, PT tensors
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
