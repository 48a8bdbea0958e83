"""Integer-lattice inputs and the exact comparison shared by tests/test_conv_exact_cpu.py and
tests/test_gpu_conv_exact.py (a helper module, not a test file).

Activations, weights and output gradients are drawn from {-1, 0, +1}.  Every such value is exact in bf16, every product
is exact, and every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order and under any
rounding mode; an output of magnitude <= 255 is exact in bf16 too.  A convolution kernel fed such operands must therefore
reproduce the float64 reference exactly -- no tolerance, so a single term dropped, doubled or taken from a neighbouring
pixel shows, however small it is next to the tensor's largest value.

`density` = P(value != 0); +1 and -1 share it equally (density 1/2: P(0) = 1/2, P(+-1) = 1/4 each).  It is an input
choice: the larger shapes lower it until the preconditions the tests assert on the reference (max |ref| <= 255,
per-channel sum of squares < 2^24) hold.
"""
import json
import os

import numpy as np
import torch

BF16_EXACT_MAX = 255          # integers of magnitude <= 255 need at most 8 significant bits: exact in bf16
F32_EXACT_BOUND = 1 << 24     # integers below 2^24 in magnitude are exact in fp32


def lattice(rng, shape, density=0.5):
  """float32 torch tensor of the given shape with values in {-1, 0, +1}, P(+1) = P(-1) = density / 2."""
  u = rng.random(tuple(shape))
  v = np.where(u < 0.5 * density, -1.0, np.where(u < density, 1.0, 0.0))
  return torch.from_numpy(v.astype(np.float32))


def exact_mismatch(got, ref):
  """The exact comparison.  None when `got` (any float dtype) equals the float64 reference `ref` element for element --
  i.e. bit for bit, a zero of either sign counting as zero -- else a message that names the first differing element's
  coordinates, both values and the number of differing elements.  NaN / inf never compare equal."""
  got = torch.as_tensor(got).detach().cpu().double()
  ref = torch.as_tensor(ref).detach().cpu().double()
  if tuple(got.shape) != tuple(ref.shape):
    return "shape %s != reference %s" % (tuple(got.shape), tuple(ref.shape))
  bad = ~(got == ref)
  n = int(bad.sum())
  if n == 0:
    return None
  idx = tuple(int(i) for i in bad.nonzero()[0])
  return "%d of %d elements differ; first at %s: got %r, reference %r (largest |difference| %g, max |reference| %g)" % (
    n, bad.numel(), idx, float(got[idx]), float(ref[idx]),
    float(torch.nan_to_num(got - ref, nan=float("inf")).abs().max()), float(ref.abs().max()))


def assert_exact(got, ref, what):
  msg = exact_mismatch(got, ref)
  assert msg is None, "%s: %s" % (what, msg)


def tolerance_accepts(got, ref, rel=1e-2):
  """The criterion of tests/test_gpu_kernels.py for the bf16 convolutions: max |got - ref| <= rel * max |ref|."""
  got = torch.as_tensor(got).double()
  ref = torch.as_tensor(ref).double()
  return float((got - ref).abs().max()) <= rel * float(ref.abs().max())


def assert_bf16_exact_range(ref, what):
  m = float(torch.as_tensor(ref).abs().max())
  assert m <= BF16_EXACT_MAX, "%s: max |reference| = %g exceeds %d -- lower the input density" % (what, m, BF16_EXACT_MAX)
  return m


def record(**figures):
  """Print the figures of a case (shape, density, largest reference magnitudes); appended to the file named by
  IIC_TEST_FIGURES as one JSON line when that variable is set."""
  line = json.dumps(figures, sort_keys=True)
  print("FIGURES " + line)
  path = os.environ.get("IIC_TEST_FIGURES")
  if path:
    with open(path, "a") as f:
      f.write(line + "\n")
