"""Non-finite values from a convolution's output to the loss, and through the Adam step: inputs with a few planted +inf,
-inf and NaN, their plain torch float64 references on the CPU, and the rule both test files apply.  Written once and used
twice, as tests/bn_bf16_cases.py and tests/conv_f64_cases.py are: tests/test_gpu_nonfinite.py runs the kernels on them,
tests/test_nonfinite_cpu.py holds every reference to the two conditions that make a case worth running --

  * at least half of the reference's outputs are finite (a kernel that writes NaN everywhere fails), and
  * every class the case is meant to show (`want`) occurs in the reference.

The rule (check): the class of every output element -- 0 finite, 1 +inf, 2 -inf, 3 NaN; NaNs are compared by class, never
by payload -- equals the reference's, and the elements the reference has finite stay within the bound the finite test of
that kernel already applies (restated or imported here, never a new one).

The finite data keep the class a matter of the reference alone: finite operands are at most 2^10 in magnitude and finite
reference outputs at most 2^20 (asserted by the CPU test), so nothing finite in float64 becomes inf in bf16 or fp32.  The
planted values sit in different channels, images or pool windows, so their regions of influence do not meet.

Two cases cannot show a +inf and say so: BatchNorm1d on batch statistics (SupHead5 in train()) turns a column that holds
any non-finite value into NaN as a whole (mean or variance is non-finite), and the stem case whose only defect is a NaN
coefficient has a finite input by definition."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.parity import U16, U32, affine_bound, bf16_rne, fma_acc_bound, pool_s2p1, rnd

NAN, INF = float("nan"), float("inf")
FIN, PINF, NINF, ISNAN = 0, 1, 2, 3
MAX_OPERAND, MAX_OUTPUT = 2.0 ** 10, 2.0 ** 20


def cls(t):
  """0 finite, 1 +inf, 2 -inf, 3 NaN."""
  v = t.detach().cpu().double()
  return torch.isposinf(v).long() + 2 * torch.isneginf(v).long() + 3 * torch.isnan(v).long()


def bf16(t):
  return t.to(torch.bfloat16).float()


def assert_classes(got, ref, what):
  bad = cls(got) != cls(ref)
  if bool(bad.any()):
    i = tuple(int(j) for j in bad.nonzero()[0])
    raise AssertionError("%s: %d of %d elements of another class than the float64 reference; first at %s: got %r, reference %r"
                         % (what, int(bad.sum()), bad.numel(), i, float(got.detach().cpu().double()[i]), float(ref.double()[i])))


def assert_finite_within(got, ref, tol, what):
  """|got - ref| <= tol on the elements the reference has finite (tol broadcasts; a non-finite tol admits anything finite)."""
  got, ref = got.detach().cpu().double(), ref.double()
  fin = cls(ref) == FIN
  tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
  bad = fin & ~((got - ref).abs() <= tol) & torch.isfinite(tol)
  if bool(bad.any()):
    i = tuple(int(j) for j in bad.nonzero()[0])
    raise AssertionError("%s: %d finite elements outside the bound; first at %s: got %r, reference %r, bound %r"
                         % (what, int(bad.sum()), i, float(got[i]), float(ref[i]), float(tol[i])))


def check(got, ref, tol, what):
  assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
  assert_classes(got, ref, what)
  assert_finite_within(got, ref, tol, what)


def assert_in_bracket_where_finite(got, ref, lo, hi, what):
  got = got.detach().cpu().double()
  fin = cls(ref) == FIN
  bad = fin & ~((lo <= got) & (got <= hi))
  assert not bool(bad.any()), "%s: %d finite elements outside their bracket" % (what, int(bad.sum()))


def _seed(*key):
  return np.random.default_rng([97] + [int(k) for k in key])


# ----------------------------------------------------------------------------------------------------------------------
# ReLU and BatchNorm apply: iic_bn_apply (bf16), iic_f32_bn_apply
# ----------------------------------------------------------------------------------------------------------------------
BN_NHWP = (2, 3, 5, 1)
BN_CS = (8, 64)
BN_MODES = ("none", "res", "y2")


@functools.lru_cache(maxsize=None)
def bn_apply_case(C, relu, mode):
  """out = [relu](scale y + shift [+ res] [+ scale2 y2 + shift2]) on [N, H, W, C] interiors holding bf16 values.  Planted,
  one channel each: 0 a NaN; 1 a +inf under a positive scale; 2 a -inf under a positive scale (0 after ReLU); 3 a +inf
  under a negative scale (-inf; 0 after ReLU); 4 a +inf whose partner in res / y2 is -inf (NaN; with neither, +inf);
  5 NaN coefficients, as a poisoned statistic leaves them: the whole channel NaN; 6 a large negative finite value (exactly
  0 after ReLU).  `zero`: the elements that must be exactly 0 with ReLU on.  A: the magnitudes of the terms, for the
  bound 6 U32 A [+ U16 |ref|] of tests/bn_bf16_cases.py check_apply_with and test_f32_bn_apply_vs_float64."""
  N, H, W, P = BN_NHWP
  rng = _seed(1, C, relu, BN_MODES.index(mode))
  y = torch.round(rnd(rng, N, H, W, C) * 8) / 8
  res, y2 = bf16(rnd(rng, N, H, W, C)), bf16(rnd(rng, N, H, W, C))
  coef, coef2 = rnd(rng, 5, C), rnd(rng, 5, C)
  coef[0, :8] = torch.tensor([0.75, 0.75, 0.5, -0.5, 1.25, 1.0, 1.0, 1.0])
  coef2[0, 4] = 0.5
  coef[1, 6] = 0.25
  y[0, 0, 0, 0] = NAN
  y[0, 1, 1, 1] = INF
  y[1, 2, 4, 2] = -INF
  y[0, 2, 3, 3] = INF
  y[1, 0, 2, 4] = INF
  if mode == "res":
    res[1, 0, 2, 4] = -INF
  if mode == "y2":
    y2[1, 0, 2, 4] = -INF
  coef[0, 5] = coef[1, 5] = NAN
  y[1, 1, 1, 6] = -1000.0
  use_res, use_y2 = mode == "res", mode == "y2"
  c, c2 = coef.double(), coef2.double()
  v = y.double() * c[0] + c[1]
  A = (y.double() * c[0]).abs() + c[1].abs()
  if use_res:
    v, A = v + res.double(), A + res.double().abs()
  if use_y2:
    v, A = v + y2.double() * c2[0] + c2[1], A + (y2.double() * c2[0]).abs() + c2[1].abs()
  ref = F.relu(v) if relu else v
  want = {ISNAN, PINF} if relu else {ISNAN, PINF, NINF}
  return dict(y=y, coef=coef, res=res if use_res else None, y2=y2 if use_y2 else None, coef2=coef2 if use_y2 else None,
              ref=ref, A=A, want=want, zero=[(1, 2, 4, 2), (0, 2, 3, 3), (1, 1, 1, 6)] if relu else [],
              operands=[y, res, y2, coef, coef2])


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm1d + ReLU of SupHead5: iic_sup_bn_relu_fwd
# ----------------------------------------------------------------------------------------------------------------------
SUP_NF = (5, 40)      # 40 features: one full 32-feature block and a ragged one of 8


@functools.lru_cache(maxsize=None)
def sup_bn_case(training):
  """x [5, 40] with a NaN (column 3), a +inf (10), a -inf (35, in the ragged block), a +inf under a negative gamma (12),
  a NaN gamma (20) and a large negative finite value (36).  On running statistics (eval) every element stands alone:
  +inf, 0, 0, NaN column, 0.  On batch statistics the column of any non-finite value is NaN as a whole -- no +inf can
  come out (module docstring).  Bound: tests/sup_head_cases.py bn_fwd_bound."""
  from tests import sup_head_cases as sh
  N, Fe = SUP_NF
  t = {k: v.clone() for k, v in sh.bn_inputs(N, Fe, 3).items()}
  x, gamma, beta = t["x"], t["gamma"], t["beta"]
  gamma[[10, 35, 36]] = 1.0
  gamma[12] = -1.0
  beta[36] = 0.0
  gamma[20] = NAN
  x[1, 3], x[0, 10], x[4, 35], x[3, 12], x[2, 36] = NAN, INF, -INF, INF, -1000.0
  r = sh.bn_ref(t, training)
  tol = sh.bn_fwd_bound(t, r)[1]
  zero = [(2, 36)] + ([] if training else [(4, 35), (3, 12)])
  return dict(t=t, ref=r["y"], tol=tol, want={ISNAN} if training else {ISNAN, PINF}, zero=zero, operands=[x, gamma, beta])


# ----------------------------------------------------------------------------------------------------------------------
# max-pools
# ----------------------------------------------------------------------------------------------------------------------
POOL_HW = ((2, 2), (6, 9), (7, 9))
POOL_BORDERS = ((1, 2), (3, 1))
POOL_N, POOL_C = 2, 8


@functools.lru_cache(maxsize=None)
def pool2_case(H, W):
  """nn.MaxPool2d(2, 2) on [N, H, W, 8] bf16 values; channels are independent, so each carries one experiment.  Channel
  q < 4: a NaN at window position q (four different windows where the image has four).  4: a +inf and a NaN in one
  window (NaN wins).  5: a window that is all -inf (-inf).  6: a NaN in the odd trailing row, which no window covers
  (odd H only: the channel stays finite).  7: a +inf alone (image 1).  The pool selects: finite outputs are bit-equal
  (tests/test_gpu_kernels_f64.py test_maxpool2_vs_torch_on_tie_dense_data)."""
  N, C = POOL_N, POOL_C
  x = bf16(rnd(_seed(2, H, W), N, H, W, C))
  Ho, Wo = H // 2, W // 2
  for q in range(4):
    yo, xo = q % Ho, (q // 2) % Wo
    x[0, 2 * yo + (q >> 1), 2 * xo + (q & 1), q] = NAN
  x[0, 0, 0, 4], x[0, 1, 1, 4] = INF, NAN
  x[0, 0:2, 0:2, 5] = -INF
  if H % 2:
    x[0, H - 1, 1, 6] = NAN
  x[1, 0, 1, 7] = INF
  ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
  return dict(x=x, ref=ref, want={ISNAN, PINF, NINF}, operands=[x])


@functools.lru_cache(maxsize=None)
def bn_pool2_case(H, W):
  """maxpool2(relu(scale y + shift)) as ops.bn_relu_maxpool2_fwd fuses it, y = pool2_case's x: positive scales on the
  planted channels (the all -inf window becomes 0) and NaN coefficients on channel 3.  The maximum is 1-Lipschitz in the
  maximum norm: a finite output is within the largest bound of its window's elements (bn_apply's 6 U32 A + U16 |ref|;
  non-finite elements and their exact images 0 / inf / NaN carry no error)."""
  x = pool2_case(H, W)["x"]
  rng = _seed(3, H, W)
  coef = rnd(rng, 5, POOL_C)
  coef[0] = torch.tensor([1.0, 0.5, 1.0, NAN, 1.0, 0.75, -1.0, 1.25])
  coef[1, 3] = NAN
  c = coef.double()
  v = x.double() * c[0] + c[1]
  a = F.relu(v)
  tol_e = 6 * U32 * ((x.double() * c[0]).abs() + c[1].abs()) + U16 * a.abs()
  tol_e = torch.where(torch.isfinite(tol_e), tol_e, torch.zeros_like(tol_e))
  pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
  return dict(y=x, coef=coef, ref=pool(a), tol=pool(tol_e), want={ISNAN, PINF}, operands=[x, coef])


@functools.lru_cache(maxsize=None)
def pool_s2p1_case(H, W):
  """nn.MaxPool2d(2, 2, padding=1) on fp32 [N, H, W, 8]: window (ho, wo) holds rows 2ho - 1, 2ho and columns 2wo - 1, 2wo
  inside the image.  Channel 0: a NaN in the corner pixel, whose window holds nothing else.  1, 2, 3: a NaN at (1, 1), in
  the last pixel and in the top right corner.  4: a NaN at (1, 1) and a +inf below it in the same window (H >= 3; NaN
  wins).  5: the window of (1, 1) all -inf.  7: a +inf alone (image 1).  Finite outputs bit-equal
  (test_f32_maxpool_s2p1_vs_torch_on_tie_dense_data)."""
  N, C = POOL_N, POOL_C
  x = rnd(_seed(4, H, W), N, H, W, C)
  x[0, 0, 0, 0] = NAN
  x[0, 1, 1, 1] = NAN
  x[0, H - 1, W - 1, 2] = NAN
  x[0, 0, W - 1, 3] = NAN
  x[0, 1, 1, 4] = NAN
  if H >= 3:
    x[0, 2, 1, 4] = INF
  x[0, 1:3, 1:3, 5] = -INF
  x[1, 0, 0, 7] = INF
  ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 2, 2, padding=1).permute(0, 2, 3, 1).contiguous()
  return dict(x=x, ref=ref, want={ISNAN, PINF, NINF}, operands=[x])


STEM_KINDS = ("pixel", "coef")
STEM_NCS = (3, 2, 8)


@functools.lru_cache(maxsize=None)
def stem_case(kind):
  """ClusterNet5g's stem (3 x 3 conv, BatchNorm coefficients, ReLU, 2 x 2 / 2 max-pool with padding 1) on [3, 2, 8, 8].
  pixel: a +inf input pixel in image 0 (its 3 x 3 neighbourhood is +-inf in every channel by the sign of weight times
  scale; every 7th channel has a negative gamma) and a NaN pixel in image 1.  coef: a finite input and NaN coefficients
  for channel 9.  Finite outputs inside parity.pooled_bracket restated with the error of a non-finite element set to 0
  (tests/first_layer_f64_cases.py stem_reference)."""
  from tests import first_layer_f64_cases as fl
  N, cin, S = STEM_NCS
  rng = _seed(5, STEM_KINDS.index(kind))
  x = rnd(rng, N, cin, S, S)
  w = rnd(rng, fl.CO, cin, 3, 3) / math.sqrt(9 * cin)
  coef = fl.stem_coefficients(F.conv2d(x.double(), w.double(), padding=1), rng)
  if kind == "pixel":
    x[0, 0, 2, 5], x[1, 1, 4, 4] = INF, NAN
  else:
    coef[0, 9] = coef[1, 9] = NAN
  y = F.conv2d(x.double(), w.double(), padding=1)
  xf = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).double()
  b = fma_acc_bound(9 * cin, F.conv2d(xf.abs(), w.double().abs(), padding=1))
  sc, sh = (coef[i].double().view(1, -1, 1, 1) for i in (0, 1))
  yf = torch.where(torch.isfinite(y), y, torch.zeros_like(y))
  z = sc * y + sh
  bz = affine_bound(yf, b, torch.nan_to_num(sc), torch.nan_to_num(sh))[1]
  bz = torch.where(torch.isfinite(z), bz, torch.zeros_like(bz))
  ref = pool_s2p1(torch.relu(z))
  lo, hi = bf16_rne(pool_s2p1(torch.relu(z - bz))), bf16_rne(pool_s2p1(torch.relu(z + bz)))
  return dict(x=x, w=w, coef=coef, ref=ref, lo=lo, hi=hi, want={ISNAN, PINF} if kind == "pixel" else {ISNAN},
              operands=[x, w, coef[:2]])


# ----------------------------------------------------------------------------------------------------------------------
# average pool, heads GEMM, softmax
# ----------------------------------------------------------------------------------------------------------------------
AVG_SHAPE = (3, 3, 5, 2, 64)      # (N, H, W, P, C): POOL_SHAPES[1] of tests/test_gpu_kernels_f64.py


@functools.lru_cache(maxsize=None)
def avgpool_case(fp32):
  """One NaN pixel poisons exactly its (n, c) feature; a +inf pixel makes its feature +inf.  Bound of
  test_avgpool_forward_backward_vs_float64: H W U32 mean |x| + U32 |ref|."""
  N, H, W, P, C = AVG_SHAPE
  x = rnd(_seed(6, fp32), N, H, W, C)
  if not fp32:
    x = bf16(x)
  x[1, 2, 3, 7], x[0, 0, 4, 40] = NAN, INF
  xd = x.double()
  ref = xd.mean((1, 2))
  tol = H * W * U32 * xd.abs().mean((1, 2)) + U32 * ref.abs()
  return dict(x=x, ref=ref, tol=tol, want={ISNAN, PINF}, operands=[x])


# one shape per kernel family behind iic_gemm_f32 (tests/test_gpu_gemm.py): the smallest tiled product, one-wave tiles,
# K-split waves, the small K-split shape, and the tiled kernel with four K-split groups
GEMM_SHAPES = ((64, 512, 256), (5, 3, 17), (32, 10, 4608), (700, 50, 4608), (700, 250, 4608))
GEMM_RUNS = ("bias", "accumulate")


@functools.lru_cache(maxsize=2)
def gemm_case(shape, run):
  """C = A B [+ bias] [+ C0].  bias (operands with the unit stride along k, as the heads' Linear has them): a NaN in one
  row of A poisons that output row, a NaN in bias one column.  accumulate (unit stride along m / n): an inf in A against a
  0 in B gives NaN in that one output and +-inf in the rest of the row, and a NaN already in C stays.  Two runs, as
  test_small_gemm_families has them: on 5 x 3 outputs the four defects together would leave fewer than half finite.
  Bound of tests/test_gpu_gemm.py: 2e-5 of the largest finite result."""
  M, N, K = shape
  g = torch.Generator().manual_seed(M * 7 + N + K + GEMM_RUNS.index(run))
  r0, r1, j1, j2, k1 = M // 2, M - 1, N - 1, 1 % N, K // 3
  if run == "bias":
    A, B, bias, C0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), None
    A[r0, K - 1] = NAN
    bias[j2] = NAN
    want = A.double() @ B.double().t() + bias.double()
    classes = {ISNAN}
  else:
    A, B, bias, C0 = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g), None, torch.randn(M, N, generator=g)
    A[k1, r1] = INF
    B[k1, j1] = 0.0
    C0[0, 0] = NAN
    want = A.double().t() @ B.double() + C0.double()
    classes = {ISNAN, PINF, NINF} if N >= 10 else {ISNAN}      # (three columns: the two infs may share a sign)
  scale = float(want[torch.isfinite(want)].abs().max())
  return dict(A=A, B=B, bias=bias, C0=C0, ref=want, tol=2e-5 * scale, want=classes, operands=[A, B] + [t for t in (bias, C0) if t is not None])


SOFTMAX_KS = (3, 16, 33, 70)
SOFTMAX_ROWS = 67


@functools.lru_cache(maxsize=None)
def softmax_case(k):
  """67 rows (a ragged last group in the grouped kernels, k <= 32; one wave per row above).  Row 5: a NaN; 9: a +inf;
  30: all -inf; 66 (the last): a NaN in the last column -- all NaN, as torch.softmax.  Row 20: -inf in columns 0 and 2 --
  those probabilities exactly 0, the rest summing to 1.  Their neighbours 4, 6, 8, 10, 19, 21, 29, 31, 65 share a wave with
  them in the grouped kernels and stay finite.  Bounds of test_softmax_rows_forward_backward: 2e-7, row sums 1e-6."""
  g = torch.Generator().manual_seed(100 + k)
  x = torch.randn(SOFTMAX_ROWS, k, generator=g) * 3
  x[5, 1], x[9, 0], x[66, k - 1] = NAN, INF, NAN
  x[30] = -INF
  x[20, 0] = x[20, 2] = -INF
  ref = torch.softmax(x.double(), 1)
  return dict(x=x, ref=ref, tol=2e-7, want={ISNAN}, zero=[(20, 0), (20, 2)], operands=[x])


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
IID_CASE = (3, 24, 10)      # (H, bn, k)
IID_LAMB = 1.5


@functools.lru_cache(maxsize=None)
def iid_case():
  """Packed sub-heads [H][bn][k] of softmax rows with one NaN probability in head 1: its raw joint has a NaN row, its
  loss and its whole gradient are NaN; heads 0 and 2 stay where they are.  loss / dz / dzt: float64 autograd through
  oracle/iid_oracle.py IID_loss per head (upstream gradient 1 on the loss, 0.5 on the loss without lambda)."""
  from oracle import iid_oracle
  from tests import iid_stage_cases as sc
  H, bn, k = IID_CASE
  f = sc.iid_f64_inputs(IID_CASE, seed=5)
  z, zt = f["z"].float().clone(), f["zt"].float().clone()
  z[1, 5, 3] = NAN
  a, b = z.double().requires_grad_(True), zt.double().requires_grad_(True)
  losses = [iid_oracle.IID_loss(a[h], b[h], lamb=IID_LAMB) for h in range(H)]
  loss, loss_nl = torch.stack([l[0] for l in losses]), torch.stack([l[1] for l in losses])
  (loss.sum() + 0.5 * loss_nl.sum()).backward()
  return dict(z=z, zt=zt, R=sc.iid_joint_ref(z, zt), loss=loss.detach(), loss_nl=loss_nl.detach(), dz=a.grad, dzt=b.grad,
              ref=torch.cat([loss.detach(), loss_nl.detach()]), want={ISNAN}, operands=[z, zt])


SEG_CASE = (2, 5, 6, 8, 1)      # (bn, k, h, w, T)


@functools.lru_cache(maxsize=None)
def seg_case(collapsed):
  """Both segmentation losses on softmax maps with one NaN pixel in x1 (inside the mask): the loss is NaN, as
  oracle/iid_oracle.py has it in float64; the same maps without the NaN give the finite loss `clean`."""
  from oracle import iid_oracle
  from oracle.gen_golden import make_seg_inputs
  bn, k, h, w, T = SEG_CASE
  x1, x2, aff, mask = make_seg_inputs(bn, k, h, w, 0.5, 0.8, 7)
  fn = iid_oracle.IID_segmentation_loss if collapsed else iid_oracle.IID_segmentation_loss_uncollapsed
  kw = dict(all_affine2_to_1=torch.from_numpy(aff).double(), all_mask_img1=torch.from_numpy(mask).double(), lamb=1.5,
            half_T_side_dense=T)
  clean = fn(torch.from_numpy(x1).double(), torch.from_numpy(x2).double(), **kw)
  x1_clean, x1 = x1, x1.copy()
  ys, xs = np.nonzero(mask[1] > 0)
  x1[1, 2, ys[len(ys) // 2], xs[len(ys) // 2]] = NAN
  bad = fn(torch.from_numpy(x1).double(), torch.from_numpy(x2).double(), **kw)
  ref = torch.stack([torch.as_tensor(float(t)) for t in bad + clean]).double()
  return dict(x1=x1, x1_clean=x1_clean, x2=x2, aff=aff, mask=mask, ref=ref, want={ISNAN}, operands=[torch.from_numpy(x1), torch.from_numpy(x2)])


@functools.lru_cache(maxsize=None)
def ce_case():
  """nn.CrossEntropyLoss on [12, 10] logits with one NaN in row 4: the mean loss is NaN and so is that row of dlogits; the
  other rows of dlogits stay within tests/sup_head_cases.py ce_bounds (computed on the logits without the NaN: the rows are
  independent)."""
  from tests import sup_head_cases as sh
  logits, targets = sh.ce_inputs(12, 10, 2, wide_row=False)
  clean = logits.clone()
  logits = logits.clone()
  logits[4, 7] = NAN
  loss, dl = sh.ce_ref(logits, targets)
  tol_dl = sh.ce_bounds(clean, targets)[1]
  return dict(logits=logits, targets=targets, loss=loss, dl=dl, tol_dl=tol_dl, ref=dl, want={ISNAN}, operands=[logits])


# ----------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 257, 70001)
ADAM_HP = tuple(float(np.float32(t)) for t in (1e-3, 0.9, 0.999, 1e-8))      # lr, beta1, beta2, eps
ADAM_STEP = 5


def adam_restated(p0, g0, m0, v0, step):
  """The kernel's expressions (csrc/optim.hip) in float64 and the bounds of
  test_adam_step_dev_vs_float64_and_the_host_counter_variant: (p, m, v) and (tol p, tol m, tol v)."""
  lr, b1, b2, eps = ADAM_HP
  s, k = lr / (1 - b1 ** step), 1 / np.sqrt(1 - b2 ** step)
  m1, v1 = b1 * m0 + (1 - b1) * g0, b2 * v0 + (1 - b2) * g0 * g0
  tm, tv = 4 * U32 * (m0.abs() + g0.abs()), 5 * U32 * (v0 + g0 * g0)
  den = v1.sqrt() * k + eps
  tden = k * tv / (2 * (v1 - tv).clamp_min(1e-300).sqrt()) + 4 * U32 * den
  upd = s * m1 / den
  tupd = s * (tm / (den - tden).clamp_min(1e-300) + m1.abs() * tden / (den - tden).clamp_min(1e-300) ** 2) + 3 * U32 * upd.abs()
  return (p0 - upd, m1, v1), (tupd + U32 * (p0.abs() + upd.abs()), tm, tv)


@functools.lru_cache(maxsize=None)
def adam_case():
  """Three tensors of 1, 257 and 70001 elements, two gradient sources each (the kernel adds them in fp32).  In the second
  and the third tensor: a NaN, a +inf and a -inf gradient, and a +inf against a -inf in the second source (NaN).  An inf
  gradient gives m = +-inf, v = +inf and p = NaN.  The reference adds the two sources in fp32 on the CPU -- the very
  IEEE addition the kernel performs, so the sum carries no error of its own -- and restates the rest in float64."""
  rng = _seed(7)
  t = {n: [rnd(rng, s) * sc for s in ADAM_SIZES] for n, sc in (("p", 1.0), ("g", 1.0), ("g2", 0.5), ("m", 0.1))}
  t["v"] = [rnd(rng, s) ** 2 * 0.01 for s in ADAM_SIZES]
  for i, at in ((1, (0, 100, 200, 256)), (2, (3, 255, 256, 70000))):
    t["g"][i][at[0]], t["g"][i][at[1]], t["g"][i][at[2]] = NAN, INF, -INF
    t["g"][i][at[3]], t["g2"][i][at[3]] = INF, -INF
  ref, tol = [], []
  for i in range(len(ADAM_SIZES)):
    g = (t["g"][i] + t["g2"][i]).double()
    r, b = adam_restated(t["p"][i].double(), g, t["m"][i].double(), t["v"][i].double(), ADAM_STEP)
    ref.append(r)
    tol.append(b)
  return dict(t=t, ref=ref, tol=tol, want=({ISNAN}, {ISNAN, PINF, NINF}, {ISNAN, PINF}),
              operands=[x for n in ("p", "g", "g2", "m", "v") for x in t[n]])


# ----------------------------------------------------------------------------------------------------------------------
# every reference, for tests/test_nonfinite_cpu.py: (name, reference outputs, classes that must occur, finite operands)
# ----------------------------------------------------------------------------------------------------------------------
def all_references():
  for C in BN_CS:
    for relu in (0, 1):
      for mode in BN_MODES:
        c = bn_apply_case(C, relu, mode)
        yield "bn_apply C=%d relu=%d %s" % (C, relu, mode), c["ref"], c["want"], c["operands"]
  for training in (True, False):
    c = sup_bn_case(training)
    yield "sup_bn training=%d" % training, c["ref"], c["want"], c["operands"]
  for H, W in POOL_HW:
    for name, fn in (("pool2", pool2_case), ("bn_pool2", bn_pool2_case), ("pool_s2p1", pool_s2p1_case)):
      c = fn(H, W)
      yield "%s %dx%d" % (name, H, W), c["ref"], c["want"], c["operands"]
  for kind in STEM_KINDS:
    c = stem_case(kind)
    yield "stem " + kind, c["ref"], c["want"], c["operands"]
  for fp32 in (False, True):
    c = avgpool_case(fp32)
    yield "avgpool fp32=%d" % fp32, c["ref"], c["want"], c["operands"]
  for shape in GEMM_SHAPES:
    for run in GEMM_RUNS:
      c = gemm_case(shape, run)
      yield "gemm %s %s" % (shape, run), c["ref"], c["want"], c["operands"]
  for k in SOFTMAX_KS:
    c = softmax_case(k)
    yield "softmax k=%d" % k, c["ref"], c["want"], c["operands"]
  c = iid_case()
  yield "iid losses", c["ref"], c["want"], c["operands"]
  yield "iid joint", c["R"], c["want"], c["operands"]
  yield "iid dz", c["dz"], c["want"], c["operands"]
  for collapsed in (False, True):
    c = seg_case(collapsed)
    yield "seg loss collapsed=%d" % collapsed, c["ref"], c["want"], c["operands"]
  c = ce_case()
  yield "cross-entropy dlogits", c["ref"], c["want"], c["operands"]
  c = adam_case()
  for j, name in enumerate(("p", "m", "v")):
    yield "adam " + name, torch.cat([r[j] for r in c["ref"]]), c["want"][j], c["operands"]
