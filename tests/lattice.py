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


# ----------------------------------------------------------------------------------------------------------------------
# First-layer, segmentation-head and fp32-GEMM cases shared by tests/test_first_layer_exact_cpu.py and
# tests/test_gpu_first_layer_exact.py: generators, float64 references with their preconditions, and the width limits of
# the stem entry points.  A power-of-two scale or a half-integer shift keeps every value a small multiple of 1/2: exact
# in fp32, and exact in bf16 whenever it survives the round trip, which the preconditions check next to the 255 bound.
# ----------------------------------------------------------------------------------------------------------------------
import torch.nn.functional as F      # noqa: E402

STEM_CO = 64
# (cin, H, W, N)
STEM_CASES = [(1, 24, 24, 3), (2, 32, 32, 3), (2, 96, 96, 2), (3, 64, 64, 2), (5, 32, 32, 3), (5, 104, 104, 2),
              (4, 6, 34, 2), (5, 2, 2, 1), (1, 4, 34, 700)]
STEM_SCALES = (1.0, -1.0, 2.0, 0.5, -2.0)
STEM_SHIFTS = (0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -3.0)
STEM_C1, STEM_C2, STEM_C3 = (1.0, -1.0, 2.0), (1.0, -1.0, 0.5, 0.0), (0.0, 1.0, -2.0)


def _draw(rng, values, n):
  return torch.tensor([values[i] for i in rng.integers(0, len(values), n)], dtype=torch.float32)


def stem_inputs(case, seed=0):
  """x, w, dpool (values on the pooled grid) from the lattice; coef [5][64] (rows 0 / 1 = scale / shift, drawn per
  channel from STEM_SCALES / STEM_SHIFTS, rows 2-4 arbitrary: the stem kernels read rows 0 and 1 only); bcoef [3][64]."""
  cin, H, W, N = case
  rng = np.random.default_rng(seed)
  x = lattice(rng, (N, cin, H, W))
  w = lattice(rng, (STEM_CO, cin, 3, 3))
  dpool = lattice(rng, (N, STEM_CO, H // 2 + 1, W // 2 + 1))
  coef = torch.cat([_draw(rng, STEM_SCALES, STEM_CO)[None], _draw(rng, STEM_SHIFTS, STEM_CO)[None],
                    torch.from_numpy(rng.standard_normal((3, STEM_CO)).astype(np.float32))])
  bcoef = torch.stack([_draw(rng, STEM_C1, STEM_CO), _draw(rng, STEM_C2, STEM_CO), _draw(rng, STEM_C3, STEM_CO)])
  return dict(case=case, x=x, w=w, dpool=dpool, coef=coef, bcoef=bcoef)


def assert_bf16_exact(ref, what):
  """|ref| <= 255 and every value survives float64 -> bf16 -> float64 (half-integers need one bit more than integers)."""
  m = assert_bf16_exact_range(ref, what)
  ref = torch.as_tensor(ref)
  assert torch.equal(ref.to(torch.bfloat16).to(ref.dtype), ref), "%s: a reference value is not a bf16 number" % what
  return m


def assert_sum_exact(terms, dims, what):
  """sum |term| over `dims` stays below 2^24 for every kept index: the fp32 sum is exact in any order."""
  m = float(terms.abs().sum(dims).max())
  assert m < F32_EXACT_BOUND, "%s: sum of magnitudes %g reaches 2^24" % (what, m)
  return m


def conv_wgrad64(x, dy, K, pad):
  """float64 weight gradient of conv2d(x, w, padding=pad) for the upstream gradient dy, by autograd."""
  w = torch.zeros((dy.shape[1], x.shape[1], K, K), dtype=torch.float64, requires_grad=True)
  F.conv2d(x.double(), w, padding=pad).backward(dy.double())
  return w.grad


def stem_reference(inp):
  """float64 torch reference of every quantity the stem kernels produce, the preconditions asserted on it.  Returns a
  dict: y, pool, sum_y, sum_yy, g (routed, ReLU-masked gradient on the conv grid), sum_g, sum_gy, dy, dW and `figures`."""
  x, w = inp["x"].double(), inp["w"].double()
  sc, sh = (inp["coef"][i].double().view(1, -1, 1, 1) for i in (0, 1))
  c1, c2, c3 = (inp["bcoef"][i].double().view(1, -1, 1, 1) for i in (0, 1, 2))
  y = F.conv2d(x, w, padding=1)
  z = (y * sc + sh).requires_grad_(True)
  a = F.relu(z)
  pool = F.max_pool2d(a, 2, 2, padding=1)
  pool.backward(inp["dpool"].double())
  g = z.grad
  dy = c1 * g + c2 * y + c3
  dW = conv_wgrad64(x, dy, 3, 1)
  fig = dict(case=list(inp["case"]))
  fig["max_y"] = assert_bf16_exact(y, "conv output (a bf16 MFMA operand of the one-pass backward)")
  fig["max_pool"] = assert_bf16_exact(a.detach(), "activation (stored as bf16 before the pool)")
  fig["max_dy"] = assert_bf16_exact(dy, "dy (a bf16 MFMA operand of the weight gradient)")
  fig["sum_abs_y"] = assert_sum_exact(y, (0, 2, 3), "sum y")
  fig["sum_yy"] = assert_sum_exact(y * y, (0, 2, 3), "sum y^2")
  fig["sum_abs_g"] = assert_sum_exact(g, (0, 2, 3), "sum g")
  fig["sum_abs_gy"] = assert_sum_exact(g * y, (0, 2, 3), "sum g*y")
  ax = x.abs()
  for name, t in (("dy", dy), ("g", g), ("y", y)):      # dW, G1, G2: per (cout, tap) sums of magnitudes
    fig["sum_abs_%s_patch" % name] = float(conv_wgrad64(ax, t.abs(), 3, 1).max())
    assert fig["sum_abs_%s_patch" % name] < F32_EXACT_BOUND, name
  fig["sum_abs_x"] = assert_sum_exact(x, (0, 2, 3), "G3")
  fig["max_dW"] = float(dW.abs().max())
  # share of pool windows whose maximum is positive and attained more than once (the routing has to pick the first)
  ap = F.pad(a.detach(), (1, 1, 1, 1), value=-1.0)
  win = torch.stack([ap[:, :, r::2, c::2] for r in (0, 1) for c in (0, 1)])
  best = win.max(0).values
  fig["tie_share"] = float((((win == best).sum(0) > 1) & (best > 0)).double().mean())
  return dict(y=y, pool=pool.detach(), sum_y=y.sum((0, 2, 3)), sum_yy=(y * y).sum((0, 2, 3)), g=g,
              sum_g=g.sum((0, 2, 3)), sum_gy=(g * y).sum((0, 2, 3)), dy=dy, dW=dW, figures=fig)


def to_pt64(x, P):
  """NCHW -> PT [N][H+2P][W+2P][C] float64 with a zero ring."""
  return F.pad(x.double(), (P, P, P, P)).permute(0, 2, 3, 1).contiguous()


# ---- stem width limits: the launch arithmetic of csrc/stem.hip and csrc/stem_bwd2.hip, restated ----------------------
LDS_BYTES = 160 * 1024        # csrc/common.h IIC_LDS_BYTES
STEM_BWD_STATIC = 5 * STEM_CO * 4      # s_cf of stem_bwd_kernel


def _a16(b):
  return (b + 15) & ~15


def stem_bwd_lds(cin, W, mode):
  """stem_bwd_lds(Cin, W, nseg, mode) of csrc/stem.hip, in bytes."""
  nseg = (W + 31) // 32
  a = 2 * W * STEM_CO * 4
  if mode >= 1:
    WP = (W + 15) & ~15
    a += _a16(STEM_CO * (2 * WP + 8) * 2) + _a16(cin * 4 * (WP + 10) * 4)
  b0 = 64 * nseg * 16 * 4
  b1 = nseg * 64 * ((cin * 9 + 31) // 32) * 32 * 4
  return max(a, b0 if mode == 0 else max(b0, b1))


def stem_width_served(entry, cin, W, bwd2=True):
  """Whether the stem entry point serves width W (even, >= 2): stem_check's W <= 256 (8 waves of 32 columns) and, for the
  backward kernels, static + dynamic LDS within the workgroup's 160 KB.  entry: "stats", "apply_pool", "bwd_reduce",
  "bwd_wgrad", "bwd_fused" (bwd2: the register-resident kernel is enabled -- it takes Cin <= 3, W <= 255)."""
  if W > 256:
    return False
  if entry in ("stats", "apply_pool"):
    return True      # apply_pool: 256 * W bytes <= 64 KB through the checked launch
  if entry == "bwd_fused" and bwd2 and cin * 9 <= 32 and W + 1 <= 256:
    return True      # at most 81 792 bytes (Cin = 3, W = 254)
  mode = {"bwd_reduce": 0, "bwd_wgrad": 1, "bwd_fused": 2}[entry]
  return stem_bwd_lds(cin, W, mode) + STEM_BWD_STATIC <= LDS_BYTES


def stem_max_width(entry, cin, bwd2=True):
  return max(W for W in range(2, 258, 2) if stem_width_served(entry, cin, W, bwd2))


# ---- first conv --------------------------------------------------------------------------------------------------------
# (cin, K, H, W, N), P = 2
FIRSTCONV_CASES = [(1, 5, 24, 24, 2), (5, 5, 24, 24, 2), (3, 5, 28, 28, 2), (4, 3, 40, 40, 2), (8, 3, 36, 32, 2),
                   (1, 3, 20, 36, 2), (2, 5, 24, 26, 2), (4, 3, 30, 30, 2), (4, 3, 200, 200, 1)]


def firstconv_inputs(case, seed=0):
  cin, K, H, W, N = case
  rng = np.random.default_rng(seed)
  return dict(case=case, x=lattice(rng, (N, cin, H, W)), w=lattice(rng, (STEM_CO, cin, K, K)),
              dy=lattice(rng, (N, STEM_CO, H, W)))


def firstconv_reference(inp):
  cin, K, H, W, N = inp["case"]
  x, w, dy = inp["x"].double(), inp["w"].double(), inp["dy"].double()
  y = F.conv2d(x, w, padding=(K - 1) // 2)
  dW = conv_wgrad64(x, dy, K, (K - 1) // 2)
  fig = dict(case=list(inp["case"]))
  fig["max_y"] = assert_bf16_exact(y, "conv output")
  fig["sum_abs_y"] = assert_sum_exact(y, (0, 2, 3), "sum y")
  fig["sum_yy"] = assert_sum_exact(y * y, (0, 2, 3), "sum y^2")
  fig["sum_abs_dy_patch"] = float(conv_wgrad64(x.abs(), dy.abs(), K, (K - 1) // 2).max())
  assert fig["sum_abs_dy_patch"] < F32_EXACT_BOUND
  fig["max_dW"] = float(dW.abs().max())
  return dict(y=y, sum_y=y.sum((0, 2, 3)), sum_yy=(y * y).sum((0, 2, 3)), dW=dW, figures=fig)


# ---- segmentation head -------------------------------------------------------------------------------------------------
# (C, k, N, Hf): every k at both C, every (N, Hf) at both weight-gradient kernels (k <= 16, k > 16)
SEG_SHAPES = [(3, 8), (3, 17), (1, 30)]
SEG_KS = [1, 3, 15, 16, 17, 24, 32]
SEG_HEAD_CASES = [(C, k, ) + SEG_SHAPES[(i + j) % 3] for j, C in enumerate((256, 512)) for i, k in enumerate(SEG_KS)]
SEG_HEAD_CASES += [(256, 16, 3, 17), (512, 32, 3, 8), (512, 3, 3, 17), (256, 24, 1, 30)]
SEG_CHAIN_CASES = [(128, 5, 3, 8), (512, 6, 3, 17)]


def seg_head_inputs(case, seed=0):
  C, k, N, Hf = case
  rng = np.random.default_rng(seed)
  return dict(case=case, f=lattice(rng, (N, C, Hf, Hf)), w=lattice(rng, (k, C, 1, 1)),
              dlog=lattice(rng, (N, k, Hf + 2, Hf + 2)))


def seg_head_reference(inp):
  """logits [M][k], dx (NCHW, the interior) and dW [k][C] of conv2d(f, w, padding=1) in float64; dlog as [M][k]."""
  C, k, N, Hf = inp["case"]
  f = inp["f"].double().requires_grad_(True)
  w = inp["w"].double().requires_grad_(True)
  out = F.conv2d(f, w, padding=1)
  out.backward(inp["dlog"].double())
  M = N * (Hf + 2) * (Hf + 2)
  logits = out.detach().permute(0, 2, 3, 1).reshape(M, k)
  dlog = inp["dlog"].double().permute(0, 2, 3, 1).reshape(M, k).contiguous()
  fig = dict(case=list(inp["case"]), M=M)
  fig["max_logit"] = float(logits.abs().max())
  assert fig["max_logit"] < F32_EXACT_BOUND
  fig["max_dx"] = assert_bf16_exact(f.grad, "feature gradient (stored as bf16)")
  fig["max_dW"] = float(w.grad.abs().max())
  assert M < F32_EXACT_BOUND      # sum of magnitudes of any column of dW <= M
  return dict(logits=logits, dlog=dlog, dx=f.grad, dW=w.grad.reshape(k, C), figures=fig)


# ---- fp32 GEMM -----------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(333, 517, 1031), (64, 512, 256), (700, 250, 4608), (32, 10, 4608), (5, 3, 17)]
SPLITK_CASE = (6, 512, 6149)      # dW[k][C] = dlog^T . F over M rows, as _SegHeadFn.backward calls it


def gemm_inputs(shape, seed=0):
  M, N, K = shape
  rng = np.random.default_rng(seed)
  return dict(A=lattice(rng, (M, K)), B=lattice(rng, (K, N)), bias=lattice(rng, (N,)), C0=lattice(rng, (M, N)))


def gemm_reference(inp, bias, accumulate):
  want = inp["A"].double() @ inp["B"].double()
  if bias:
    want = want + inp["bias"].double()
  if accumulate:
    want = want + inp["C0"].double()
  assert inp["A"].shape[1] + 2 < F32_EXACT_BOUND      # |C| <= K + 2: every partial sum is an exact fp32 integer
  return want
